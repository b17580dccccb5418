"""GPU tier: zc_ris_double_and_compress through the C ABI against the oracle's ris_compress(ed_double(P)).  Host arrays and
device tensors, every launch form of the shared inversions (one row per lane, chunked with ragged last lanes, the two forms the
host picks by size), all point classes interleaved with hostile rows, framed buffers (no byte outside the output rows and no
input byte changes, and nothing around the rows reaches a result), and the k/2 mod L recipe."""
import ctypes as C

import numpy as np
import pytest

from oracle import pymodel as pm
from tests import framed_buffers as FB
from tests import hostile_rows as H
from tests import point_classes as PC
from tests import vectors as V

pytestmark = pytest.mark.gpu

SEED = V.SEED + 0xDAC0
NAME = "zc_ris_double_and_compress"
HOSTILE_EVERY = 17


@pytest.fixture(scope="module")
def eng():
    import dusk_zerocaf_amd as z
    e = z.Engine()
    yield e
    e.close()


def dev(x):
    import torch
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x if x.dtype == np.uint8 else x.view(np.int64)).cuda()


def host(t):
    a = t.cpu().numpy()
    return a if a.dtype == np.uint8 else a.view(np.uint64)


@pytest.fixture(scope="module")
def cat(oracle):
    """(rows, expected, hostile patterns): every class of tests/point_classes.classes(oracle, 64, seed) interleaved and
    [0..15] B -- 464 curve points with the oracle's encodings of their doubles, computed once -- and the hostile point records."""
    rows, names = PC.interleave(PC.classes(oracle, 64, SEED))
    mult = [pm.IDENT]
    for _ in range(15):
        mult.append(pm.ed_add(mult[-1], pm.BASEPOINT))
    rows = np.ascontiguousarray(np.concatenate([rows, V.pts_np(mult)]))
    want = oracle.ris_compress(oracle.ed_double(rows))
    e8 = [i for i, nm in enumerate(names) if nm == "torsion"] + [len(names)]
    assert not want[e8].any() and want[[i for i, nm in enumerate(names) if nm == "subgroup"]].any(axis=1).all()
    hostile = np.array([w for _, w in H.point_patterns(rows[1])], dtype=np.uint64)
    for x in (rows, want, hostile):
        x.setflags(write=False)
    return rows, want, hostile


def batch(cat, n, c=1):
    """n rows: the catalogue in turn, a hostile record at every 17th row from row 5 and at the rows
    tests/hostile_rows.hostile_set(n, c) constructs from the launch geometry.  Returns (rows, expected, mask of the curve points)."""
    rows, want, hostile = cat
    idx = np.arange(n) % len(rows)
    a, w = rows[idx], want[idx]
    hs = sorted(set(range(5, n, HOSTILE_EVERY)) | (set(H.hostile_set(n, c)) if n >= 64 else set()))
    for j, i in enumerate(hs):
        a[i] = hostile[j % len(hostile)]
    return a, w, H.clean_mask(n, hs)


def raw(e, p_ptr, out_ptr, n):
    from dusk_zerocaf_amd import _lib
    _lib.check(getattr(e.lib, NAME)(e.ctx, C.c_void_p(p_ptr), C.c_void_p(out_ptr), n), NAME, e.lib)


def both_places(e, a, w, good, what):
    """Host arrays and device tensors: every curve point gets the oracle's bytes, and the two places agree on every row."""
    h = e.ris_double_and_compress(a)
    assert isinstance(h, np.ndarray) and h.shape == (len(a), 32) and h.dtype == np.uint8
    bad = np.flatnonzero((h != w).any(axis=1) & good)
    assert len(bad) == 0, "%s, host arrays: rows %s differ from the oracle" % (what, bad[:16])
    d = host(e.ris_double_and_compress(dev(a)))
    assert np.array_equal(d, h), "%s: host arrays and device tensors differ in rows %s" % (what, np.flatnonzero((d != h).any(axis=1))[:16])
    return h


@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_one_row_per_lane_under_default_tuning(eng, cat, n):
    a, w, good = batch(cat, n)
    both_places(eng, a, w, good, "n = %d" % n)


@pytest.mark.parametrize("n", [300, 301])
@pytest.mark.parametrize("c", [2, 7, 32])
def test_shared_inversions_with_ragged_last_lanes(cat, c, n):
    a, w, good = batch(cat, n, c)
    with V.tuned(ZC_INV_CHUNK=c) as te:
        both_places(te, a, w, good, "n = %d, %d rows per lane" % (n, c))


@pytest.mark.parametrize("n", [131072, 131149], ids=["lone", "chunked"])
def test_the_forms_the_host_picks_by_size(eng, cat, n):
    """131072 rows are the first the host shares inversions for by itself (two per lane) and, on 256 compute units, the last
    whose 65536 lanes leave one wave per SIMD: k_ris_double_compress_chunked_lone.  131149 rows (65575 lanes) take
    k_ris_double_compress_chunked."""
    a, w, good = batch(cat, n, 2)
    got = host(eng.ris_double_and_compress(dev(a)))
    bad = np.flatnonzero((got != w).any(axis=1) & good)
    assert len(bad) == 0, "rows %s differ from the oracle" % bad[:16]


def test_rows_off_the_curve_get_the_same_bytes_in_every_form(cat):
    """The whole output, hostile rows included, is the same with one row per lane and with seven."""
    a, w, good = batch(cat, 301, 7)
    out = {}
    for c in (1, 7):
        with V.tuned(ZC_INV_CHUNK=c) as te:
            out[c] = both_places(te, a, w, good, "%d rows per lane" % c)
    assert np.array_equal(out[1], out[7]), np.flatnonzero((out[1] != out[7]).any(axis=1))[:16]
    assert (~good).sum() >= 17


def test_no_rows_is_no_call(eng):
    import torch
    p, out = dev(np.zeros((4, 20), dtype=np.uint64)), torch.full((4, 32), 0xEE, dtype=torch.uint8, device="cuda")
    raw(eng, p.data_ptr(), out.data_ptr(), 0)
    torch.cuda.synchronize()
    assert (host(out) == 0xEE).all()
    hp, hout = np.zeros((4, 20), dtype=np.uint64), np.full((4, 32), 0xEE, dtype=np.uint8)
    raw(eng, hp.ctypes.data, hout.ctypes.data, 0)
    assert (hout == 0xEE).all()
    assert eng.ris_double_and_compress(np.zeros((0, 20), dtype=np.uint64)).shape == (0, 32)


@pytest.mark.parametrize("backend", ["torch", "numpy"])
def test_framed_buffers_no_byte_outside_the_rows(oracle, cat, backend):
    """n = 300 at seven rows per lane: the prefix products wait in the output rows themselves, so the frames around them and
    every input byte must be as they were, with zero and with hostile frames, rows on a 16-byte boundary and 8 bytes off one;
    the outputs are the same under both fills, and the curve points get the oracle's bytes."""
    import torch
    n = 300
    a, w, good = batch(cat, n, 7)
    frames = FB.hostile_frame_rows("pt", oracle)
    with V.tuned(ZC_INV_CHUNK=7) as te:
        if backend == "torch":
            te._follow_torch_stream(torch.empty(1, dtype=torch.uint8, device="cuda"))

        def call(ip, op):
            raw(te, ip[0], op[0], n)
            torch.cuda.synchronize()
            te.synchronize()
        got = {}
        for fill in (FB.ZERO, FB.HOSTILE):
            for shift in (0, 8):
                res = FB.run_framed(call, [("p", a, frames)], [("out32", n, 32, np.uint8)], backend=backend, fill=fill, in_shifts=[shift], out_shifts=[shift])
                got[fill, shift] = res
                bad = np.flatnonzero((res[0] != w).any(axis=1) & good)
                assert len(bad) == 0, (fill, shift, bad[:16])
        for shift in (0, 8):
            FB.same_outputs(["out32"], got[FB.ZERO, shift], got[FB.HOSTILE, shift], "%s, rows %d bytes off" % (NAME, shift))
        FB.same_outputs(["out32"], got[FB.ZERO, 0], got[FB.ZERO, 8], "%s, aligned and offset rows" % NAME)


def test_half_the_scalar_then_double_and_compress(eng, oracle):
    """For 256 points of the subgroup and random k: the encoding of k P is ris_double_and_compress((k / 2 mod L) P), with the
    halved scalar from zc_sc_muladd (b = 2^-1 mod L) and the windowed multiplication."""
    from dusk_zerocaf_amd import engine
    n = 256
    P = dev(PC.subgroup(oracle, n, SEED + 1))
    k = V.rand_scalars_np(n, SEED + 2, bits=249)
    half = np.tile(np.array(pm.limbs((pm.L + 1) // 2), dtype=np.uint64), (n, 1))
    k2 = eng.sc_muladd(dev(k), dev(half), dev(np.zeros((n, 5), dtype=np.uint64)))
    assert [pm.from_limbs(r) for r in host(k2)[:8]] == [pm.from_limbs(r) * ((pm.L + 1) // 2) % pm.L for r in k[:8]]
    got = host(eng.ris_double_and_compress(eng.ed_scalar_mul(P, k2, flags=engine.FAST)))
    want = host(eng.ris_compress(eng.ed_scalar_mul(P, dev(k), flags=engine.STRICT)))
    assert np.array_equal(got, want) and want.any(axis=1).all()
    assert np.array_equal(want, oracle.ris_compress(oracle.mt(oracle.ed_scalar_mul, host(P), k)))
