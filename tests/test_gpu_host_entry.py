"""GPU tier: the host side of the batched entry points (zerocaf_hip.hip: `batched` over typed row buffers, run_batched) --
optional accept masks passed as NULL, and a launch that reports a failure from any chunk, any worker thread and the
device-resident path."""
import ctypes as C

import numpy as np
import pytest

from tests import vectors as V

pytestmark = pytest.mark.gpu

N = 300                                     # two workgroups, the second partial
ZC_ERR_NOMEM = -4


@pytest.fixture(scope="module")
def eng():
    import dusk_zerocaf_amd as z
    e = z.Engine()
    yield e
    e.close()


def eq(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


@pytest.fixture(scope="module")
def rows(eng):
    """Inputs of N rows in which some rows fail every op's own acceptance test, computed once."""
    rng = np.random.default_rng(V.SEED + 0x3A5)
    fe_a, fe_b = V.rand_fe_np(N, V.SEED + 0x3A6), V.rand_fe_np(N, V.SEED + 0x3A7)
    fe_a[::7] = 0                           # not invertible
    fe_b[3::5] = 0
    pts = eng.ed_mul_base(V.rand_scalars_np(N, V.SEED + 0x3A8, bits=249))
    bad_pts = pts.copy()
    bad_pts[::6, 10:15] = 0                 # Z = 0: no affine form, no encoding
    enc = eng.ris_compress(pts)
    junk = rng.integers(0, 256, size=(N, 32), dtype=np.uint8)
    ed_enc = eng.ed_compress(pts)[0]
    ed_enc[::3] = junk[::3]                 # about half of random encodings are off the curve
    ris_enc = enc.copy()
    ris_enc[::4] = junk[::4]
    sc_bytes = junk.copy()
    sc_bytes[::2, 31] = 0                   # below the group order; nearly all of the others are at or above it
    terms = np.stack([ris_enc, np.roll(enc, 1, axis=0)], axis=1).copy()
    return {"fe_a": fe_a, "fe_b": fe_b, "bad_pts": bad_pts, "ed_enc": ed_enc, "ris_enc": ris_enc, "sc_bytes": sc_bytes,
            "k": V.rand_scalars_np(N, V.SEED + 0x3A9, bits=252), "terms": terms,
            "k2": V.rand_scalars_np(2 * N, V.SEED + 0x3AA, bits=252).reshape(N, 2, 5), "kb": V.rand_scalars_np(N, V.SEED + 0x3AB, bits=252)}


U64, U8 = np.uint64, np.uint8
# symbol -> (input names, by-value arguments between inputs and outputs, (width, dtype) of the outputs before the mask)
MASKED = {
    "zc_fe_invert": (["fe_a"], (), [(5, U64)]),
    "zc_fe_div": (["fe_a", "fe_b"], (), [(5, U64)]),
    "zc_fe_mod_sqrt": (["fe_a"], (C.c_int(1),), [(5, U64)]),
    "zc_fe_sqrt_ratio_i": (["fe_a", "fe_b"], (), [(5, U64)]),
    "zc_fe_inv_sqrt": (["fe_a"], (), [(5, U64)]),
    "zc_sc_from_bytes": (["sc_bytes"], (), [(5, U64)]),
    "zc_ed_to_affine": (["bad_pts"], (), [(10, U64)]),
    "zc_ed_compress": (["bad_pts"], (), [(32, U8)]),
    "zc_ed_decompress": (["ed_enc"], (), [(20, U64)]),
    "zc_ris_decompress": (["ris_enc"], (), [(20, U64)]),
    "zc_ris_roundtrip_mul": (["ris_enc", "k"], (), [(32, U8)]),
    "zc_ris_lincomb": (["terms", "k2"], (2, None), [(32, U8)]),                    # base_scalars absent as well
    "zc_ris_lincomb+base": (["terms", "k2", "kb"], (), [(32, U8)]),
}


@pytest.mark.parametrize("case", sorted(MASKED))
def test_optional_masks_may_be_null(eng, rows, case):
    """Every entry point with an optional accept mask, called through ctypes with the mask NULL, on host arrays and on device
    tensors: ZC_OK, and the other outputs are those of the call that takes the mask -- rows the mask rejects included."""
    import torch
    names, mid, outs = MASKED[case]
    fn = getattr(eng.lib, case.split("+")[0])
    ins = [rows[k] for k in names]
    if case.endswith("+base"):                                                     # (in32, scalars, terms, base_scalars, out32, ok, n)
        ins, tail_in = ins[:2], [ins[2]]
        mid = (2,)
    else:
        tail_in = []

    def call(arrays, mask, like=None):
        res = [np.full((N, w), 0xEE, dtype=dt) for w, dt in outs]
        if like is not None:
            res = [torch.from_numpy(r.view(np.int64) if r.dtype == U64 else r).cuda() for r in res]
        ptr = lambda x: x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()
        base = [ptr(x) for x in arrays[len(ins):]]
        rc = fn(eng.ctx, *[ptr(x) for x in arrays[:len(ins)]], *mid, *base, *[ptr(r) for r in res], None if mask is None else ptr(mask), N)
        assert rc == 0, eng.lib.zc_last_error()
        if like is not None:
            torch.cuda.synchronize()
            res = [r.cpu().numpy().view(dt) for r, (_, dt) in zip(res, outs)]
        return res

    mask = np.full(N, 0xEE, dtype=U8)
    want = call(ins + tail_in, mask)
    assert set(np.unique(mask)) == {0, 1}, "the inputs must hold rows the mask rejects and rows it accepts"
    got = call(ins + tail_in, None)
    assert all(eq(g, w) for g, w in zip(got, want)), case + ": host arrays"
    dev = [torch.from_numpy(x.view(np.int64) if x.dtype == U64 else x).cuda() for x in ins + tail_in]
    eng._follow_torch_stream(dev[0])
    got = call(dev, None, like=dev[0])
    assert all(eq(g, w) for g, w in zip(got, want)), case + ": device tensors"
    eng.use_own_stream()


def test_a_failed_launch_ends_the_call_with_its_status_from_any_chunk(eng, oracle):
    """A launch functor that reports a failure (here: the test build refuses the second launch of every device job on the
    host, ZC_TEST_LAUNCH_FAIL=2; no kernel is involved) must end the call with that status and message, although the chunks
    before and -- before the functors returned a status -- after it succeed.  A call of one chunk on the same context works."""
    import dusk_zerocaf_amd as z
    n = 4096                                                                       # ZC_HOST_CHUNKS=4: four chunks of 1024 rows
    a, b = V.rand_fe_np(n, V.SEED + 0x3B0), V.rand_fe_np(n, V.SEED + 0x3B1)
    K = V.rand_scalars_np(n, V.SEED + 0x3B2, bits=252)
    P = np.tile(V.base_multiples(oracle, 1024, V.SEED + 0x3B3), (4, 1))
    with V.tuned(hooks=True, ZC_HOST_CHUNKS=4, ZC_TEST_LAUNCH_FAIL=2) as te:
        for what in (lambda: te.fe_mul(a, b), lambda: te.ed_scalar_mul(P, K, flags=z.FAST)):
            with pytest.raises(z.ZerocafHipError, match="launch refused") as ei:
                what()
            assert "status %d " % ZC_ERR_NOMEM in str(ei.value)
        out = np.empty_like(a)
        assert te.lib.zc_fe_mul(te.ctx, a.ctypes.data, b.ctypes.data, out.ctypes.data, n) == ZC_ERR_NOMEM
        assert te.lib.zc_last_error() == b"test: launch refused"
        assert eq(te.fe_mul(a[:1024], b[:1024]), oracle.fe_mul(a[:1024], b[:1024]))          # one chunk: one launch
        fast = te.ed_scalar_mul(P[:1024], K[:1024], flags=z.FAST)
        assert eq(oracle.ed_compress(fast)[0], oracle.ed_compress(oracle.ed_scalar_mul(P[:1024], K[:1024]))[0])


def test_a_failed_launch_is_reported_from_worker_threads_and_for_device_buffers(eng):
    """Two device slots: each shard of a host batch runs on a thread of its own, and the message a worker sets (thread-local)
    must reach the caller with the status.  Device-resident buffers: the status of the one launch is the call's."""
    import dusk_zerocaf_amd as z
    import torch
    n = 4096                                                                       # two shards of 2048 rows, two chunks each
    a, b = V.rand_fe_np(n, V.SEED + 0x3B4), V.rand_fe_np(n, V.SEED + 0x3B5)
    with V.tuned(hooks=True, devices=[0, 0], ZC_HOST_CHUNKS=2, ZC_TEST_LAUNCH_FAIL=2) as te:
        assert te.lib.zc_fe_mul(te.ctx, None, b.ctypes.data, a.ctypes.data, n) != 0          # another message on this thread first
        with pytest.raises(z.ZerocafHipError, match="launch refused") as ei:
            te.fe_mul(a, b)
        assert "status %d " % ZC_ERR_NOMEM in str(ei.value)
        assert eq(te.fe_mul(a[:2048], b[:2048]), eng.fe_mul(a[:2048], b[:2048]))             # one chunk per shard
    with V.tuned(hooks=True, ZC_TEST_LAUNCH_FAIL=1) as te:
        dA, dB = (torch.from_numpy(x.view(np.int64)).cuda() for x in (a, b))
        with pytest.raises(z.ZerocafHipError, match="launch refused") as ei:
            te.fe_mul(dA, dB)
        assert "status %d " % ZC_ERR_NOMEM in str(ei.value)
        torch.cuda.synchronize()
