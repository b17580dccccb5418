"""GPU tier: no entry point writes or reads outside the rows it is given.

Every batched entry point of tests/entry_table.py is called through the C ABI with pointers into the MIDDLE of larger
allocations (tests/framed_buffers.py: [front frame | rows | back frame]), as a caller does who passes a sub-range of a device
array.  After the call the memory is read back:
  a. every output frame is intact, every input (frames and rows) is byte-identical to before, and the output rows -- 0xEE before
     the call -- are what the oracle says (limbs, or the group element where the header promises no more; those entries also
     give the limbs of a call on plain compact buffers);
  b. outputs and masks are byte-identical whether the input frames hold zeros or hostile rows of the buffer's type: no
     neighbour reaches a result;
  c. the same with the rows on a 16-byte boundary (the staged forms) and 8 bytes off one (the per-lane forms); byte arrays 8
     off, flag bytes 3 off, and the inputs of zc_sc_from_bytes_wide / _mod_order 1 off;
  d. every launch form at the smallest size that reaches it, proved by the test build's launch counter where there is one;
  e. host pointers: framed numpy buffers through one device slot, two slots, and forced chunks with a partial last chunk.
Nothing here can fault: an overrun lands in a frame of the same allocation, and is found there."""
import time

import numpy as np
import pytest

from tests import entry_table as T
from tests import framed_buffers as FB
from tests import lincomb_rows as LR
from tests import vectors as V

pytestmark = pytest.mark.gpu

UNALIGNED_BYTES = ("zc_sc_from_bytes_wide", "zc_sc_from_bytes_mod_order")      # tests/test_gpu_scalar_ext.py: inputs at any address
FLAG_SHIFT = 3                                                                 # masks and flags are single bytes
assert 300 % 7 == 6 and 301 % 2 == 1                                           # T.INV_SIZES under T.INV_CHUNKS: a ragged last lane, a last lane of one row


@pytest.fixture(scope="module")
def g(oracle):
    return T.Gen(oracle)


def bind(e):
    """Device calls of `e` run on torch's current stream, where the framed buffers are filled and read."""
    import torch
    e._follow_torch_stream(torch.empty(1, dtype=torch.uint8, device="cuda"))
    return e


@pytest.fixture(scope="module")
def eng():
    import dusk_zerocaf_amd as z
    e = z.Engine()
    yield bind(e)
    e.close()


def inputs_of(g, e, n):
    return [T.rows_of(i.gen(g), n * i.per_n) for i in e.ins]


def bases_of(g, e, n):
    return T.rows_of(e.bases.gen(g), n) if e.bases else None


def want_of(g, e, n):
    """The oracle's outputs for n rows: computed once per entry on the POOL rows and repeated, or once per size where a row
    of the output is a sum over the batch."""
    if e.rowwise:
        pool = g.memo(("want", e.id), lambda: [np.ascontiguousarray(w) for w in e.want(g, *[np.ascontiguousarray(i.gen(g)) for i in e.ins])])
        return [T.rows_of(w, n) for w in pool]
    kw = {"bases": bases_of(g, e, n)} if e.bases else {}
    return g.memo(("want", e.id, n), lambda: [np.ascontiguousarray(w) for w in e.want(g, *inputs_of(g, e, n), **kw)])


def hostile(g, kind):
    return g.memo(("hostile", kind), lambda: FB.hostile_frame_rows(kind, g.oracle))


def shifts_for(e, bufs, shifted):
    """Row starts relative to a 16-byte boundary: 0 everywhere, or 8 for u64 arrays and byte records (1 for the two entry
    points that take bytes at any address), 3 for flag bytes."""
    if not shifted:
        return [0] * len(bufs)
    out = []
    for b in bufs:
        if b.dtype == T.U64:
            out.append(8)
        elif b.width == 0:
            out.append(FLAG_SHIFT)
        else:
            out.append(1 if e.symbol in UNALIGNED_BYTES and isinstance(b, T.In) else 8)
    return out


class Runner:
    """Calls of one engine on framed or compact buffers; counts the staged launches of the test build per call."""

    def __init__(self, eng, g):
        self.eng, self.g = eng, g
        self.hooks = hasattr(eng.lib, "zc_test_staged_launches")
        self.staged = []                                   # per call: launches that took a staged kernel (test build)

    def _invoke(self, e, in_ptrs, out_ptrs, n, table_id):
        import torch
        c0 = self.eng.lib.zc_test_staged_launches(self.eng.ctx) if self.hooks else 0
        rc = getattr(self.eng.lib, e.symbol)(self.eng.ctx, *e.args(in_ptrs, out_ptrs, n, table_id))
        assert rc == 0, (e.id, n, self.eng.lib.zc_last_error())
        torch.cuda.synchronize()
        self.eng.synchronize()
        self.staged.append((self.eng.lib.zc_test_staged_launches(self.eng.ctx) - c0) if self.hooks else None)

    def table(self, e, n, backend, fill, shifted):
        """zc_msm_fixed: its table, created from framed points (which must stay as they were); the id lands in a framed word."""
        import ctypes as C
        pts = FB.FramedBuffer("input 'points' of zc_msm_bases_create", bases_of(self.g, e, n), backend,
                              0 if fill == FB.ZERO else hostile(self.g, e.bases.kind), 8 if shifted else 0)
        word = FB.FramedBuffer("output 'id_out'", np.zeros((1, 1), dtype=np.uint64), "numpy", FB.OUT_FRAME_FILL, 8 if shifted else 0)
        rc = self.eng.lib.zc_msm_bases_create(self.eng.ctx, pts.ptr, n, 0, C.cast(word.ptr, C.POINTER(C.c_uint64)))
        assert rc == 0, self.eng.lib.zc_last_error()
        import torch
        torch.cuda.synchronize()
        pts.assert_unchanged()
        word.assert_frames_intact()
        return int(word.rows()[0, 0])

    def framed(self, e, n, fill, shifted, backend="torch", alias=None):
        ins = inputs_of(self.g, e, n)
        out_backend = "numpy" if e.place == "host" else backend
        table_id = self.table(e, n, backend, fill, shifted) if e.bases else None
        try:
            return FB.run_framed(lambda ip, op: self._invoke(e, ip, op, n, table_id),
                                 [(e.id + ": " + i.name, a, hostile(self.g, i.kind)) for i, a in zip(e.ins, ins)],
                                 [(e.id + ": " + o.name, e.out_rows(j, n), o.width, o.dtype) for j, o in enumerate(e.outs)],
                                 backend=backend, fill=fill, in_shifts=shifts_for(e, e.ins, shifted), out_shifts=shifts_for(e, e.outs, shifted),
                                 alias=alias, out_backend=out_backend)
        finally:
            if table_id:
                self.eng.lib.zc_msm_bases_destroy(self.eng.ctx, table_id)

    def compact(self, e, n, backend="torch"):
        """The same call on plain whole allocations."""
        import ctypes as C
        import torch
        ins = inputs_of(self.g, e, n)
        shapes = [(e.out_rows(j, n), o.width) if o.width else (e.out_rows(j, n),) for j, o in enumerate(e.outs)]
        outs = [np.full(int(np.prod(sh)) * o.dtype.itemsize, FB.OUT_ROW_FILL, dtype=np.uint8).view(o.dtype).reshape(sh) for sh, o in zip(shapes, e.outs)]
        dev = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()
        out_dev = backend == "torch" and e.place != "host"
        d_in = [dev(a) if backend == "torch" else a for a in ins]
        d_out = [dev(a) if out_dev else a for a in outs]
        ptr = lambda x: x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data
        table_id = None
        if e.bases:
            bases = bases_of(self.g, e, n)
            d_b = dev(bases) if backend == "torch" else bases
            word = C.c_uint64(0)
            assert self.eng.lib.zc_msm_bases_create(self.eng.ctx, ptr(d_b), n, 0, C.byref(word)) == 0, self.eng.lib.zc_last_error()
            table_id = word.value
        try:
            self._invoke(e, [ptr(x) for x in d_in], [ptr(x) for x in d_out], n, table_id)
        finally:
            if table_id:
                self.eng.lib.zc_msm_bases_destroy(self.eng.ctx, table_id)
        return [x.cpu().numpy().view(o.dtype).reshape(a.shape) if out_dev else a for x, a, o in zip(d_out, outs, e.outs)]


def assert_want(g, e, got, want, what):
    names = [o.name for o in e.outs]
    if e.equal == "limbs":
        for nm, x, w in zip(names, got, want):
            w = np.asarray(w).reshape(x.shape)
            bad = np.flatnonzero((x.reshape(len(x), -1) != w.reshape(len(w), -1)).any(axis=1))
            assert len(bad) == 0, "%s: output '%s' differs from the oracle in rows %s" % (what, nm, bad[:16])
    else:
        LR.assert_same_points(g.oracle, got[0], want[0])


def check_entry(run, e, n, backend="torch"):
    """a, b and c for one entry at one size.  Returns {form: outputs}."""
    g = run.g
    want = want_of(g, e, n)
    names = [o.name for o in e.outs]
    what = "%s, n = %d" % (e.id, n)
    res = {"compact": run.compact(e, n, backend)}
    assert_want(g, e, res["compact"], want, what + ", compact buffers")
    for form, fill, shifted in (("zero frames, aligned", FB.ZERO, False), ("hostile frames, aligned", FB.HOSTILE, False),
                                ("zero frames, offset", FB.ZERO, True), ("hostile frames, offset", FB.HOSTILE, True)):
        res[form] = run.framed(e, n, fill, shifted, backend)
        if e.equal == "limbs":
            assert_want(g, e, res[form], want, what + ", " + form)
        FB.same_outputs(names, res["compact"], res[form], what + ": compact buffers and " + form)
    FB.same_outputs(names, res["zero frames, aligned"], res["hostile frames, aligned"], what + ", aligned rows")
    FB.same_outputs(names, res["zero frames, offset"], res["hostile frames, offset"], what + ", offset rows")
    return res


def sizes_of(e):
    return tuple(sorted(set(T.STD_SIZES + e.sizes)))


# ------------------------------------------------------------------ a, b, c at the default sizes (and each entry's own)
@pytest.mark.parametrize("case", sorted(T.TABLE))
def test_rows_only(eng, g, case):
    """Frames intact, inputs untouched, values exact, neighbours without influence, rows aligned and offset: every entry at
    n = 1, 255, 257 and 300; the windowed core also on both sides of one wave (63, 65); the MSM family also at the smallest
    size that takes the bucket pipeline (and zc_msm_batch below its own threshold), as the plan queries confirm."""
    e = T.TABLE[case]
    run = Runner(eng, g)
    t0 = time.perf_counter()
    for n in sizes_of(e):
        if e.symbol in ("zc_msm", "zc_msm_partial"):
            assert (eng.msm_plan(n)["window_bits"] > 0) == (n >= T.MSM_BUCKET_MIN_N), n
        if e.symbol == "zc_msm_batch":
            assert (eng.msm_batch_plan(n, T.MSM_BATCH)["regime"] == "buckets") == (n >= T.MSM_BATCH_BUCKET_MIN_N), n
        check_entry(run, e, n)
    print("%s: sizes %s, %.2f s" % (case, sizes_of(e), time.perf_counter() - t0))


@pytest.mark.parametrize("case", sorted(k for k, e in T.TABLE.items() if e.mask is not None))
def test_null_mask_on_framed_buffers(eng, g, case):
    """The optional mask passed as NULL: the other outputs are unchanged and nothing outside the rows is written."""
    e = T.TABLE[case]
    n = 300
    want = want_of(g, e, n)
    ins = inputs_of(g, e, n)
    import torch

    def call(ip, op):
        rc = getattr(eng.lib, e.symbol)(eng.ctx, *e.args(ip, op, n, null_mask=True))
        assert rc == 0, eng.lib.zc_last_error()
        torch.cuda.synchronize()
    got = FB.run_framed(call, [(case + ": " + i.name, a, hostile(g, i.kind)) for i, a in zip(e.ins, ins)],
                        [(case + ": " + o.name, n, o.width, o.dtype) for o in e.outs], backend="torch", fill=FB.HOSTILE)
    assert (got[e.mask] == FB.OUT_ROW_FILL).all(), "the mask buffer was written although NULL was passed"
    for j, (x, w) in enumerate(zip(got, want)):
        if j != e.mask:
            assert np.array_equal(x, np.asarray(w).reshape(x.shape)), (case, e.outs[j].name)


# ------------------------------------------------------------------ d. every launch form
@pytest.mark.parametrize("case", T.STAGED_40_ENTRIES)
def test_staged_40_byte_kernels(g, case):
    """ZC_TEST_STREAM_MIN_BYTES=1 (test build): add, sub, neg, mul and square, field and scalar, move their 40-byte records
    through LDS at every size when the arrays are 16-byte aligned (coop_load40 / coop_store40 patch the odd last word), and
    take the per-lane kernel when they are 8 bytes off.  The launch counter says which form produced what was compared."""
    e = T.TABLE[case]
    with V.tuned(hooks=True, ZC_TEST_STREAM_MIN_BYTES=1) as te:
        run = Runner(bind(te), g)
        for n in T.STD_SIZES:
            check_entry(run, e, n)
        assert run.staged == [1, 1, 1, 0, 0] * len(T.STD_SIZES), run.staged        # compact, two aligned, two offset
    print("%s: staged form reached at n = %s (launch counter)" % (case, T.STD_SIZES))


@pytest.mark.parametrize("case", T.STAGED_POINT_ENTRIES)
def test_staged_point_kernels(g, case):
    """Above 2^12 points add, sub, double and neg stage their 160-byte records with a workgroup size of their own: 4097 rows
    (one row into the last workgroup) and 4397."""
    e = T.TABLE[case]
    with V.tuned(hooks=True) as te:
        run = Runner(bind(te), g)
        check_entry(run, e, T.ED_STAGED_MIN_POINTS)                                 # the threshold itself: per lane
        assert run.staged == [0] * 5, run.staged
        run.staged = []
        for n in T.STAGED_POINT_SIZES:
            check_entry(run, e, n)
        assert run.staged == [1, 1, 1, 0, 0] * len(T.STAGED_POINT_SIZES), run.staged
    print("%s: staged form reached at n = %s (launch counter)" % (case, T.STAGED_POINT_SIZES))


@pytest.mark.parametrize("chunk", T.INV_CHUNKS)
@pytest.mark.parametrize("case", T.SHARED_INVERSION_ENTRIES)
def test_chunked_shared_inversions(g, case, chunk):
    """ZC_INV_CHUNK = 2 and 7 at 300 and 301 rows: lanes own `chunk` rows and park prefix products in the output records; the
    last lane is ragged (300 = 42 * 7 + 6) or holds one row (301 = 150 * 2 + 1 = 43 * 7).  Then once more with the output
    aliasing an input where the header allows it (one inversion per row): the frames of that buffer stay intact."""
    e = T.TABLE[case]
    with V.tuned(ZC_INV_CHUNK=chunk) as te:
        run = Runner(bind(te), g)
        for n in T.INV_SIZES:
            check_entry(run, e, n)
            want = want_of(g, e, n)
            for j, i in e.alias:
                for fill in (FB.ZERO, FB.HOSTILE):
                    for shifted in (False, True):
                        got = run.framed(e, n, fill, shifted, alias={j: i})
                        assert_want(g, e, got, want, "%s, n = %d, output '%s' aliasing input '%s'" % (case, n, e.outs[j].name, e.ins[i].name))
    print("%s: chunked form at ZC_INV_CHUNK=%d, n = %s (by size constants)" % (case, chunk, T.INV_SIZES))


@pytest.fixture(scope="module")
def strict_big(oracle):
    """The repeated 1024-point pool of tests/test_gpu_ctx_lifecycle.py under fresh 252-bit scalars, 2^17 + 77 rows."""
    n = T.PW_MIN_ELEMS + 77
    pool = V.base_multiples(oracle, 1024, V.SEED + 900)
    P = np.ascontiguousarray(np.tile(pool, (n // 1024 + 1, 1))[:n])
    K = V.rand_scalars_np(n, T.SEED + 902, bits=252)
    K[0], K[1], K[n - 1] = 0, V.raw_scalar_edges()[1], V.raw_scalar_edges()[2]
    return P, K


def strict_case(run, g, P, K, rows, what):
    """The strict scalar-mul on framed rows P, K: all rows against the compact call, the rows `rows` against the oracle."""
    e = T.TABLE["zc_ed_scalar_mul[STRICT]"]
    n = len(P)
    want = g.oracle.mt(g.oracle.ed_scalar_mul, np.ascontiguousarray(P[rows]), np.ascontiguousarray(K[rows]))
    inputs = [(what + ": p", P, hostile(g, "pt")), (what + ": k", K, hostile(g, "sc"))]
    outputs = [(what + ": out", n, 20, T.U64)]
    call = lambda ip, op: run._invoke(e, ip, op, n, None)
    import torch
    dP, dK = (torch.from_numpy(a.view(np.int64)).cuda() for a in (P, K))
    dO = torch.full((n, 20), -1, dtype=torch.int64, device="cuda")
    call([dP.data_ptr(), dK.data_ptr()], [dO.data_ptr()])
    compact = dO.cpu().numpy().view(np.uint64)
    assert np.array_equal(compact[rows], want), what + ": compact buffers differ from the oracle"
    res = []
    for fill, shift in ((FB.ZERO, 0), (FB.HOSTILE, 0), (FB.HOSTILE, 8)):
        got = FB.run_framed(call, inputs, outputs, backend="torch", fill=fill, in_shifts=[shift] * 2, out_shifts=[shift])
        FB.same_outputs(["out"], [compact], got, "%s: compact buffers and %s frames, rows %d bytes off" % (what, fill, shift))
        res.append(got)
    FB.same_outputs(["out"], res[0], res[1], what)


@pytest.mark.parametrize("n", [T.QUAD_LAUNCH_ELEMS - 1, T.QUAD_LAUNCH_ELEMS + 1])
def test_strict_scalar_mul_both_sides_of_the_quad_launch(eng, g, n):
    """2^14 - 1 rows take four lanes per row, 2^14 + 1 one lane per row: every row against the oracle."""
    P = T.rows_of(g.points(), n)
    K = V.rand_scalars_np(n, T.SEED + 910 + n, bits=252)
    K[:T.POOL] = g.raw_sc(1)
    strict_case(Runner(eng, g), g, P, K, np.arange(n), "strict scalar-mul, n = %d" % n)
    print("strict scalar-mul: %s form at n = %d (by size constant QUAD_LAUNCH_ELEMS)" % ("four-lane" if n <= T.QUAD_LAUNCH_ELEMS else "one-lane", n))


def test_strict_scalar_mul_block_schedule(g):
    """ZC_SCHED=block at 300 rows."""
    e = T.TABLE["zc_ed_scalar_mul[STRICT]"]
    with V.tuned(ZC_SCHED="block") as te:
        check_entry(Runner(bind(te), g), e, 300)
    print("strict scalar-mul: ZC_SCHED=block at n = 300")


def test_strict_scalar_mul_cost_sorted_form(eng, g, strict_big):
    """2^17 + 77 rows: persistent waves walk the cost-sorted permutation; a ragged last tile.  Every 2053rd row against the
    oracle (as tests/test_gpu_ctx_lifecycle.py), all rows against the compact call."""
    P, K = strict_big
    rows = np.unique(np.r_[np.arange(0, len(P), 2053), len(P) - 1])
    strict_case(Runner(eng, g), g, P, K, rows, "strict scalar-mul, n = 2^17 + 77")
    print("strict scalar-mul: cost-sorted persistent form at n = %d (by size constant PW_MIN_ELEMS)" % len(P))


# ------------------------------------------------------------------ e. host pointers
HOST_ENTRIES = ("zc_fe_mul", "zc_ed_add", "zc_ris_decompress", "zc_ed_coset4", "zc_ed_scalar_mul[STRICT]", "zc_msm_batch", "zc_msm_fixed")
HOST_CONFIGS = {                                            # name -> (devices, ZC_HOST_CHUNKS, n)
    "one slot": (None, None, 300),
    "two slots": ([0, 0], None, 301),
    "three chunks, the last partial": (None, 3, 2500),     # chunks are whole multiples of 1024 rows: 1024 + 1024 + 452
    "two slots, uneven shards in chunks": ([0, 0], 3, 2501),
}


@pytest.mark.parametrize("config", sorted(HOST_CONFIGS))
@pytest.mark.parametrize("case", HOST_ENTRIES)
def test_host_buffers(g, case, config):
    """Framed numpy buffers: what the download writes into the caller's memory is rows 0 .. n - 1 and nothing else, through one
    device slot, two, and chunked staging with a partial last chunk; the values are the oracle's.  (For the two MSM entries
    the host buffer the library writes is out_points; n is the instance size and stays small.)"""
    devices, chunks, n = HOST_CONFIGS[config]
    e = T.TABLE[case]
    if not e.rowwise:
        n = 300 if devices is None and chunks is None else 301 if chunks is None else 70 + (devices is not None)
    with V.tuned(devices=devices, ZC_HOST_CHUNKS=chunks) as te:
        run = Runner(te, g)
        want = want_of(g, e, n)
        names = [o.name for o in e.outs]
        got = {}
        for fill in (FB.ZERO, FB.HOSTILE):
            for shifted in (False, True):
                got[fill, shifted] = run.framed(e, n, fill, shifted, backend="numpy")
                assert_want(g, e, got[fill, shifted], want, "%s, %s, n = %d" % (case, config, n))
        for shifted in (False, True):
            FB.same_outputs(names, got[FB.ZERO, shifted], got[FB.HOSTILE, shifted], "%s, %s" % (case, config))
