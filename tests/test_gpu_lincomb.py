"""GPU tier: zc_ed_lincomb, out[i] = sum_j k[i][j] * P[i][j] with one doubling chain per row (through the C ABI).

Every expected value is composed from the oracle's own Mul<Scalar> and Add in index order (tests/lincomb_rows.py); a row
passes as the same group element with the same compressed Edwards and Ristretto bytes.  All rows are compared."""
import ctypes as C

import numpy as np
import pytest

from tests import lincomb_rows as R
from tests import vectors as V

pytestmark = pytest.mark.gpu

ZC_OK, ZC_ERR_BAD_ARG, ZC_ERR_MIXED_MEM = 0, -1, -5
FAST = 16


@pytest.fixture(scope="module")
def eng():
    import dusk_zerocaf_amd as z
    e = z.Engine()
    yield e
    e.close()


def gpu_points(e):
    """count subgroup points r_i * B, computed by the fixed-base comb (not the code under test)."""
    return lambda count, seed: e.ed_mul_base(V.rand_scalars_np(count, seed, bits=249))


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def to_host(t):
    return t.cpu().numpy().view(np.uint64)


def composition(e, P, K):
    """What the library offered before: one windowed multiplication per term on contiguous copies, folded with ed_add."""
    t = P.shape[1]
    acc = None
    for j in range(t):
        q = e.ed_scalar_mul(P[:, j].contiguous(), K[:, j].contiguous(), flags=FAST)
        acc = q if acc is None else e.ed_add(acc, q)
    return acc


@pytest.mark.parametrize("t", range(1, 9))
def test_row_families_vs_oracle(eng, oracle, t):
    """5000 rows with every planted family (zero scalars, 1, L, L - 1, all-ones limbs, raw patterns >= 2^256, identity /
    equal / opposite points, mixed bit lengths, the three points ed_coset4 adds to the identity), host arrays."""
    n = 5000
    P, K, where = R.lincomb_rows(oracle, n, t, V.SEED + 2000 + 10 * t, points=gpu_points(eng))
    assert len(where) >= 60
    got = eng.ed_lincomb(P, K)
    assert got.shape == (n, 20) and got.dtype == np.uint64
    R.assert_same_points(oracle, got, R.oracle_lincomb(oracle, P, K))


@pytest.mark.parametrize("t", [2, 5, 8])
def test_device_tensors_match_host_arrays_limb_for_limb(eng, oracle, t):
    """Device tensors in, device tensor out, on torch's current stream -- the default one and a side stream -- without
    the call waiting for the device; the limbs are those of the host-array call (deterministic)."""
    import torch
    n = (1 << 16) + 77
    P, K, _ = R.lincomb_rows(oracle, n, t, V.SEED + 2100 + t, points=gpu_points(eng))
    host = eng.ed_lincomb(P, K)
    dP, dK = to_dev(P), to_dev(K)
    warm = eng.ed_lincomb(dP, dK)                                    # the first device call may allocate
    torch.cuda.synchronize()
    out = eng.ed_lincomb(dP, dK)
    pending = not torch.cuda.current_stream().query()                # the call returned with its kernel still in flight
    torch.cuda.synchronize()
    assert pending
    assert out.is_cuda and tuple(out.shape) == (n, 20)
    assert np.array_equal(to_host(out), host) and np.array_equal(to_host(warm), host)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        sP, sK = to_dev(P), to_dev(K)                                # produced on the side stream
        out2 = eng.ed_lincomb(sP, sK)                                # follows it
        pending = not side.query()
    side.synchronize()
    assert pending and np.array_equal(to_host(out2), host)
    torch.cuda.synchronize()
    stride = np.random.default_rng(V.SEED + 2101).choice(n, 4096, replace=False)
    R.assert_same_points(oracle, host[stride], R.oracle_lincomb(oracle, P[stride], K[stride]))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, (1 << 14) + 5, (1 << 16) + 300])
def test_launch_shapes(eng, oracle, n):
    """Partial waves, partial workgroups, one workgroup more than a power of two -- t = 2, against the oracle on every row
    up to 2^14 + 5 and on head, tail and a seeded 4096-row subset above."""
    t = 2
    P = gpu_points(eng)(n * t, V.SEED + 2200 + n).reshape(n, t, 20)
    K = V.rand_scalars_np(n * t, V.SEED + 2201 + n, bits=252).reshape(n, t, 5)
    K[n // 2] = 0
    K[-1, 0] = [(1 << 52) - 1] * 5
    got = eng.ed_lincomb(P, K)
    if n <= (1 << 14) + 5:
        rows = np.arange(n)
    else:
        pick = np.random.default_rng(V.SEED + 2202).choice(n, 4096, replace=False)
        rows = np.unique(np.concatenate([np.arange(300), np.arange(n - 300, n), pick]))
        assert len(rows) >= 4096
    R.assert_same_points(oracle, got[rows], R.oracle_lincomb(oracle, P[rows], K[rows]))


@pytest.mark.parametrize("log_n,t", [(20, 2), (18, 8)])
def test_large_batches_on_the_device(eng, oracle, log_n, t):
    """2^20 rows of two terms and 2^18 rows of eight, device-resident: every row ed_eq (on the device) to the composition
    of the windowed multiplication and ed_add, every output a valid point, a seeded 4096-row subset against the oracle."""
    import torch
    n = 1 << log_n
    dP = eng.ed_mul_base(to_dev(V.rand_scalars_np(n * t, V.SEED + 2300 + t, bits=249))).reshape(n, t, 20)
    K = V.rand_scalars_np(n * t, V.SEED + 2301 + t, bits=252).reshape(n, t, 5)
    K[5] = 0
    K[n - 1, t - 1] = [(1 << 52) - 1] * 5
    dK = to_dev(K)
    got = eng.ed_lincomb(dP, dK)
    want = composition(eng, dP, dK)
    eq = eng.ed_eq(got, want)
    ok = eng.ed_is_valid(got)
    torch.cuda.synchronize()
    assert bool(eq.all()) and bool(ok.all())
    rows = np.unique(np.concatenate([[0, 5, n - 1], np.random.default_rng(V.SEED + 2302).choice(n, 4096, replace=False)]))
    idx = torch.from_numpy(rows).cuda()
    R.assert_same_points(oracle, to_host(got[idx]), R.oracle_lincomb(oracle, to_host(dP[idx]), K[rows]))


@pytest.mark.parametrize("slots", [100, 7, 1])
def test_ring_under_contention(eng, oracle, slots):
    """ZC_RING_SLOTS below the number of resident waves, a single-digit value and 1: waves queue for their multi-unit
    slots, the limbs are those of the default ring, twice in a row (the ring state is reset per launch), and the other
    users of the shared ring on the same context are not disturbed."""
    n = 1 << 13
    cases = {}
    for t in (2, 8):
        P, K, _ = R.lincomb_rows(oracle, n, t, V.SEED + 2400 + t, points=gpu_points(eng))
        cases[t] = (P, K, eng.ed_lincomb(P, K))
    P1, K1 = np.ascontiguousarray(cases[2][0][:, 0]), np.ascontiguousarray(cases[2][1][:, 0])
    enc = oracle.mt(oracle.ris_compress, P1)
    fast_ref, rt_ref = eng.ed_scalar_mul(P1, K1, flags=FAST), eng.ris_roundtrip_mul(enc, K1)
    with V.tuned(ZC_RING_SLOTS=slots) as e:
        assert np.array_equal(e.ed_scalar_mul(P1, K1, flags=FAST), fast_ref)
        for t in (2, 8, 2):
            P, K, ref = cases[t]
            assert np.array_equal(e.ed_lincomb(P, K), ref)
            assert np.array_equal(e.ed_lincomb(P, K), ref)
            rt = e.ris_roundtrip_mul(enc, K1)
            assert np.array_equal(rt[0], rt_ref[0]) and np.array_equal(rt[1], rt_ref[1])
            assert np.array_equal(e.ed_scalar_mul(P1, K1, flags=FAST), fast_ref)
    for t in (2, 8):
        P, K, ref = cases[t]
        R.assert_same_points(oracle, ref, R.oracle_lincomb(oracle, P, K))


def test_argument_errors(eng, oracle):
    lib, ctx = eng.lib, eng.ctx
    P = np.ascontiguousarray(gpu_points(eng)(16, V.SEED + 2500)).reshape(2, 8, 20)
    K = V.rand_scalars_np(16, V.SEED + 2501).reshape(2, 8, 5)
    out = np.full((2, 20), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    before = out.copy()
    call = lambda p, k, t, o, n: lib.zc_ed_lincomb(ctx, p, k, t, o, n)
    assert call(P.ctypes.data, K.ctypes.data, 0, out.ctypes.data, 2) == ZC_ERR_BAD_ARG
    assert call(P.ctypes.data, K.ctypes.data, 9, out.ctypes.data, 1) == ZC_ERR_BAD_ARG
    assert call(P.ctypes.data, K.ctypes.data, 2, out.ctypes.data, 1 << 30) == ZC_ERR_BAD_ARG        # n * terms = 2^31
    assert call(None, K.ctypes.data, 2, out.ctypes.data, 1) == ZC_ERR_BAD_ARG
    assert lib.zc_ed_lincomb(None, P.ctypes.data, K.ctypes.data, 2, out.ctypes.data, 1) == ZC_ERR_BAD_ARG
    assert call(P.ctypes.data, K.ctypes.data, 8, out.ctypes.data, 0) == ZC_OK
    assert np.array_equal(out, before)                               # n == 0 and the failures above wrote nothing
    dK = to_dev(K)
    assert call(P.ctypes.data, dK.data_ptr(), 8, out.ctypes.data, 2) == ZC_ERR_MIXED_MEM
    assert np.array_equal(out, before)
    with pytest.raises(AssertionError):
        eng.ed_lincomb(P, K[:1])
    assert eng.ed_lincomb(P[:0], K[:0]).shape == (0, 20)
    got = eng.ed_lincomb(P, K)                                       # the context is as usable as before
    R.assert_same_points(oracle, got, R.oracle_lincomb(oracle, P, K))
