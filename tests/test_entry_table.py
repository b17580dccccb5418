"""CPU tier: the entry table (tests/entry_table.py) covers include/zerocaf_hip.h, and the framed-buffer checks
(tests/framed_buffers.py) can fail.

The GPU tier cannot plant a bug in a kernel, so the second half runs the very checks of tests/test_gpu_buffer_bounds.py on the
numpy backend against a "library" of a few lines of Python with one defect each: a byte written after the last row, a write
into the front frame, a modified input row, an output that depends on the first frame row.  Each must be reported with the
right buffer, side and offset."""
import os

import numpy as np
import pytest

from dusk_zerocaf_amd import _lib
from tests import entry_table as T
from tests import framed_buffers as FB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "zerocaf_hip.h")).read()


# ------------------------------------------------------------------ the table against the header
def test_every_function_of_the_header_is_in_the_table_or_excluded_with_a_reason():
    missing, unknown, both = T.coverage_gaps(HEADER)
    assert not missing, "entry points that tests/entry_table.py neither describes nor excludes: %s" % missing
    assert not unknown, "names the header does not declare: %s" % unknown
    assert not both
    assert all(isinstance(r, str) and len(r) > 5 for r in T.EXCLUDED.values())
    assert len(T.prototypes(HEADER)) == len(_lib.ALL_SYMBOLS) == len(set(n for n, _ in T.prototypes(HEADER)))


def test_nothing_that_takes_row_buffers_is_excluded():
    """An excluded function has no `const uint64_t *` / `const uint8_t *` array argument followed by a row count -- except the
    two named ones: zc_msm_sharded (needs a communicator) and zc_comm_init (its 128 bytes are an id, not rows)."""
    for name, args in T.prototypes(HEADER):
        if name in T.EXCLUDED and name not in ("zc_msm_sharded", "zc_comm_init"):
            assert "const uint64_t *" not in args and "const uint8_t *" not in args, (name, args)


def test_a_removed_entry_is_noticed():
    table = {k: v for k, v in T.TABLE.items() if v.symbol != "zc_ed_coset4"}
    assert T.coverage_gaps(HEADER, table)[0] == ["zc_ed_coset4"]
    table = {k: v for k, v in T.TABLE.items() if v.symbol != "zc_msm_fixed"}
    assert T.coverage_gaps(HEADER, table)[0] == ["zc_msm_bases_create", "zc_msm_fixed"]


def test_a_new_prototype_is_noticed():
    new = HEADER.replace("int zc_ed_coset4(", "int zc_ed_coset8(zc_ctx *ctx, const uint64_t *p, uint64_t *out8, size_t n);\nint zc_ed_coset4(")
    assert new != HEADER
    assert T.coverage_gaps(new)[0] == ["zc_ed_coset8"]


def test_the_argument_settings_the_table_must_hold():
    ids = set(T.TABLE)
    want = ["zc_ed_scalar_mul[%s]" % f for f in ("STRICT", "LTR_BIN", "BINARY_NAF", "FAST")]
    want += ["zc_sc_compute_naf[width=%d]" % w for w in (0, 2, 7)] + ["zc_sc_shr[shift=%d]" % s for s in (0, 1, 255)]
    want += ["zc_fe_mod_sqrt[sign=%d]" % s for s in (0, 1)] + ["zc_ed_mul_by_pow_2[kexp=%d]" % k for k in (0, 1, 249)]
    want += ["zc_ed_mul_base_wnaf[width=%d]" % w for w in (2, 7)] + ["zc_ed_lincomb[terms=%d]" % t for t in (1, 3, 8)]
    want += ["zc_ris_lincomb[terms=1]", "zc_ris_lincomb[terms=8]", "zc_ris_lincomb[terms=1,base]", "zc_ris_lincomb[terms=7,base]"]
    want += ["zc_msm", "zc_msm_partial", "zc_ed_fold_ordered", "zc_msm_fixed", "zc_msm_batch"]
    assert not [w for w in want if w not in ids]
    for name in ("zc_msm", "zc_msm_partial", "zc_msm_fixed", "zc_msm_batch"):
        assert T.MSM_BUCKET_MIN_N in T.TABLE[name].sizes and T.MSM_BATCH == 3
    for e in T.TABLE.values():
        if e.symbol in ("zc_ris_roundtrip_mul", "zc_ed_lincomb", "zc_ris_lincomb") or e.id == "zc_ed_scalar_mul[FAST]":
            assert set(T.CORE_SIZES) <= set(e.sizes), e.id
    assert T.LINCOMB_MAX_TERMS == int(HEADER.split("#define ZC_LINCOMB_MAX_TERMS")[1].split()[0])


def test_the_table_matches_the_ctypes_signatures():
    """Every entry's argument list has the length of the bound signature, pointers where that has pointers."""
    import ctypes as C
    sigs = dict(_lib.SIGNATURES, **_lib.SCALAR_EXT_SIGNATURES)
    for e in T.TABLE.values():
        args = e.args(list(range(1000, 1000 + len(e.ins))), list(range(2000, 2000 + len(e.outs))), 7, table_id=5)
        sig = sigs[e.symbol]
        assert len(args) == len(sig), e.id
        for a, t in zip(args, sig):
            if t is C.c_void_p:
                assert a is None or isinstance(a, int) and a >= 1000, (e.id, a)
            elif t is C.c_size_t and not isinstance(a, int):
                assert isinstance(a, C.c_size_t), (e.id, a)
            elif t is not C.c_size_t:
                assert isinstance(a, t), (e.id, a, t)
        assert e.mask is None or e.outs[e.mask].width == 0


def test_frames_are_large_enough_and_hold_hostile_rows(oracle):
    for rb in (1, 32, 40, 64, 160, 640, 1280):
        f = FB.frame_bytes(rb)
        assert f >= 64 << 10 and f >= 256 * rb and f % 16 == 0
    from oracle import pymodel as pm
    from tests import hostile_rows as HR
    fe = FB.hostile_frame_rows("fe")
    assert any((r == HR.ALL_ONES).all() for r in fe) and any(r.tolist() == pm.limbs(pm.P) for r in fe)
    sc = FB.hostile_frame_rows("sc")
    assert any(r.tolist() == pm.limbs(pm.L) for r in sc) and any(HR.value(r) >= 1 << 256 for r in sc)
    pt = FB.hostile_frame_rows("pt")
    assert any(HR.zero_by_value(r[10:15]) and r[:10].any() for r in pt)
    enc = FB.hostile_frame_rows("enc32", oracle)
    assert (oracle.ris_decompress(enc)[1] == 0).any() and (oracle.ed_decompress(enc)[1] == 0).any()
    assert FB.hostile_frame_rows("pt*3").shape[1] == 60 and FB.hostile_frame_rows("enc32*8", oracle).shape[1] == 256
    for e in T.TABLE.values():
        for i in e.ins:
            rows = FB.hostile_frame_rows(i.kind, oracle)
            assert rows.shape[1] == i.width and rows.dtype == i.dtype, (e.id, i.name)
    # the frame rows lie on the row grid on both sides, at every shift
    rows = np.arange(15, dtype=np.uint64).reshape(3, 5) + 100
    for shift in (0, 8):
        b = FB.FramedBuffer("x", rows, "numpy", fe, shift)
        img = b.read()
        assert b.ptr % 16 == shift and np.array_equal(b.rows(), rows)
        after = img[b.front + b.nbytes:b.front + b.nbytes + 40].view(np.uint64)
        assert np.array_equal(after, fe[0])
        before = img[b.front - 40:b.front].view(np.uint64)
        assert any(np.array_equal(before, r) for r in fe)


# ------------------------------------------------------------------ the checks can fail: a Python "library" with one defect each
N, W = 300, 5


def fake_add(defect=None):
    """out = a + b over rows of five u64 words, through raw addresses like the C ABI."""
    def call(in_ptrs, out_ptrs):
        a = FB.host_bytes(in_ptrs[0], N * W * 8).view(np.uint64).reshape(N, W)
        b = FB.host_bytes(in_ptrs[1], N * W * 8).view(np.uint64).reshape(N, W)
        out = FB.host_bytes(out_ptrs[0], N * W * 8).view(np.uint64).reshape(N, W)
        out[:] = a + b
        if defect == "one byte after the last row":
            FB.host_bytes(out_ptrs[0] + N * W * 8, 1)[0] = 0x5A
        elif defect == "a row before the first":
            FB.host_bytes(out_ptrs[0] - 40, 40)[:] = 0x11
        elif defect == "writes an input row":
            b[7, 2] ^= np.uint64(1)
        elif defect == "reads the row before the first":
            out[0] += FB.host_bytes(in_ptrs[0] - 40, 40).view(np.uint64)
        elif defect == "reads the row after the last":
            out[N - 1] += FB.host_bytes(in_ptrs[1] + N * W * 8, 40).view(np.uint64)
    return call


def run_fake(defect, fill, shift=0):
    rng = np.random.default_rng(5)
    a, b = (rng.integers(0, 1 << 52, size=(N, W), dtype=np.uint64) for _ in range(2))
    hostile = FB.hostile_frame_rows("fe")
    got = FB.run_framed(fake_add(defect), [("a", a, hostile), ("b", b, hostile)], [("out", N, W, np.uint64)], backend="numpy", fill=fill,
                        in_shifts=[shift] * 2, out_shifts=[shift])
    return got, [a + b]


@pytest.mark.parametrize("shift", [0, 8])
def test_a_correct_library_passes(shift):
    zero, want = run_fake(None, FB.ZERO, shift)
    host, _ = run_fake(None, FB.HOSTILE, shift)
    assert np.array_equal(zero[0], want[0])
    FB.same_outputs(["out"], zero, host)


@pytest.mark.parametrize("shift", [0, 8])
def test_one_byte_after_the_last_row_is_caught(shift):
    with pytest.raises(FB.FrameError) as ei:
        run_fake("one byte after the last row", FB.ZERO, shift)
    err = ei.value
    assert (err.buffer, err.side, err.first, err.last, err.count, err.found[0]) == ("output 'out'", "back", 0, 0, 1, 0x5A)
    assert "output 'out'" in str(err) and "after the last row" in str(err) and "+0 .. +0" in str(err) and "5a" in str(err)


def test_a_write_into_the_front_frame_is_caught():
    with pytest.raises(FB.FrameError) as ei:
        run_fake("a row before the first", FB.HOSTILE)
    err = ei.value
    assert (err.buffer, err.side, err.first, err.last, err.count) == ("output 'out'", "front", -40, -1, 40) and err.found[:2] == [0x11, 0x11]


def test_a_modified_input_row_is_caught():
    with pytest.raises(FB.FrameError) as ei:
        run_fake("writes an input row", FB.ZERO)
    err = ei.value
    assert (err.buffer, err.side, err.first, err.last, err.count) == ("input 'b'", "rows", 7 * 40 + 16, 7 * 40 + 16, 1)


@pytest.mark.parametrize("defect,row", [("reads the row before the first", 0), ("reads the row after the last", N - 1)])
def test_an_output_that_depends_on_a_frame_row_is_caught(defect, row):
    zero, want = run_fake(defect, FB.ZERO)                 # with zero frames the defect is invisible: the values are right
    assert np.array_equal(zero[0], want[0])
    host, _ = run_fake(defect, FB.HOSTILE)                 # no frame changed, no input changed
    with pytest.raises(FB.NeighbourLeak) as ei:
        FB.same_outputs(["out"], zero, host, "fake add")
    assert (ei.value.buffer, ei.value.row, ei.value.count) == ("out", row, 1)
    assert "out" in str(ei.value) and "first row %d" % row in str(ei.value)
