"""GPU tier: zc_ris_lincomb, out32[i] = compress(kB[i] * B + sum_j k[i][j] * decompress(in32[i][j])) (through the C ABI).

Every expected value is composed from the oracle's own decompress, Mul<Scalar>, Add and compress (tests/ris_lincomb_rows.py);
all 32 bytes and the accept mask are compared, on every row unless a test says which."""
import numpy as np
import pytest

from oracle import pymodel as pm
from tests import ris_lincomb_rows as RR
from tests import vectors as V

pytestmark = pytest.mark.gpu

ZC_OK, ZC_ERR_BAD_ARG, ZC_ERR_MIXED_MEM = 0, -1, -5
POOL = (1 << 14) + 5


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
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.dtype == np.uint8 else a.view(np.int64)).cuda()


def to_host(t):
    a = t.cpu().numpy()
    return a if a.dtype == np.uint8 else a.view(np.uint64)


def rows_for(eng, oracle, n, t, seed, base):
    return RR.ris_lincomb_rows(oracle, n, t, seed, base, points=gpu_points(eng), compress=eng.ris_compress)


@pytest.mark.parametrize("t,base", RR.CASES)
def test_row_families_vs_oracle(eng, oracle, t, base):
    """5000 host rows: the encodings of every planted scalar and point family, every family of undecodable encoding in
    every term position (a zero scalar on it included), the planted base scalars."""
    n = 5000
    E, K, KB, planted = rows_for(eng, oracle, n, t, V.SEED + 4000 + 10 * t + int(base), base)
    got, ok = eng.ris_lincomb(E, K, KB)
    assert got.shape == (n, 32) and got.dtype == np.uint8 and ok.shape == (n,) and ok.dtype == np.uint8
    RR.assert_same_bytes((got, ok), RR.oracle_ris_lincomb(oracle, E, K, KB))
    assert 0 < int((ok == 0).sum()) <= planted and not got[ok == 0].any()


_pools = {}


def pool(eng, oracle, t):
    """POOL rows of t terms and a base term with the oracle's bytes, computed once and left unchanged."""
    if t not in _pools:
        E = eng.ris_compress(gpu_points(eng)(POOL * t, V.SEED + 4100 + t)).reshape(POOL, t, 32)
        K = V.rand_scalars_np(POOL * t, V.SEED + 4101 + t, bits=252).reshape(POOL, t, 5)
        KB = V.rand_scalars_np(POOL, V.SEED + 4102 + t, bits=252)
        _pools[t] = (E, K, KB) + RR.oracle_ris_lincomb(oracle, E, K, KB)
    return _pools[t]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 129, 255, 257, POOL])
@pytest.mark.parametrize("t", [2, 5])
def test_launch_shapes(eng, oracle, t, n):
    """Partial waves and partial workgroups of the 256-lane (2 terms + base) and the 128-lane (5 terms + base) launch; the
    last row is undecodable, a middle row has all-zero scalars; every row against the oracle."""
    E, K, KB, want, wok = (a[:n].copy() for a in pool(eng, oracle, t))
    mid = n // 2
    K[mid], KB[mid] = 0, 0
    E[n - 1, t - 1] = RR.le32(pm.P - int.from_bytes(bytes(E[n - 1, t - 1]), "little"))
    patched = sorted({mid, n - 1})
    want[patched], wok[patched] = RR.oracle_ris_lincomb(oracle, E[patched], K[patched], KB[patched])
    assert wok[n - 1] == 0 and (n == 1 or (wok[mid] == 1 and not want[mid].any()))
    RR.assert_same_bytes(eng.ris_lincomb(E, K, KB), (want, wok))


@pytest.mark.parametrize("t", [1, 7])
def test_device_tensors_match_host_arrays(eng, oracle, t):
    """Device tensors in, device tensors out, on torch's current stream -- the default one and a side stream -- without the
    call waiting for the device; bytes and mask are those of the host-array call; ok = NULL is accepted."""
    import torch
    n = (1 << 16) + 77
    E, K, KB, _ = rows_for(eng, oracle, n, t, V.SEED + 4200 + t, True)
    host, host_ok = eng.ris_lincomb(E, K, KB)
    dE, dK, dKB = to_dev(E), to_dev(K), to_dev(KB)
    warm = eng.ris_lincomb(dE, dK, dKB)                              # the first device call may allocate
    torch.cuda.synchronize()
    out, ok = eng.ris_lincomb(dE, dK, dKB)
    pending = not torch.cuda.current_stream().query()                # the call returned with its kernel still in flight
    torch.cuda.synchronize()
    assert pending
    assert out.is_cuda and tuple(out.shape) == (n, 32) and ok.is_cuda and tuple(ok.shape) == (n,)
    RR.assert_same_bytes((to_host(out), to_host(ok)), (host, host_ok))
    RR.assert_same_bytes((to_host(warm[0]), to_host(warm[1])), (host, host_ok))
    bare = torch.full((n, 32), 0xA5, dtype=torch.uint8, device="cuda")
    assert eng.lib.zc_ris_lincomb(eng.ctx, dE.data_ptr(), dK.data_ptr(), t, dKB.data_ptr(), bare.data_ptr(), None, n) == ZC_OK
    torch.cuda.synchronize()
    assert np.array_equal(to_host(bare), host)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        sE, sK, sKB = to_dev(E), to_dev(K), to_dev(KB)               # produced on the side stream
        out2, ok2 = eng.ris_lincomb(sE, sK, sKB)                     # follows it
        pending = not side.query()
    side.synchronize()
    assert pending
    RR.assert_same_bytes((to_host(out2), to_host(ok2)), (host, host_ok))
    torch.cuda.synchronize()
    pick = np.unique(np.concatenate([np.arange(300), np.random.default_rng(V.SEED + 4201).choice(n, 4096, replace=False)]))
    RR.assert_same_bytes((host[pick], host_ok[pick]), RR.oracle_ris_lincomb(oracle, E[pick], K[pick], KB[pick]))
    assert 0 < int((host_ok[pick] == 0).sum())


def test_consistency_with_the_existing_surface(eng, oracle):
    """On the device, byte for byte: one term without a base term is ris_roundtrip_mul; one term under a zero scalar with a
    base term is ris_mul_base_compress on decodable rows; t terms with a base term are
    ris_compress(ed_add(ed_lincomb(ris_decompress ...), ed_mul_base)) on decodable rows and zeros elsewhere."""
    import torch
    n, t = 1 << 14, 3
    E, K, KB, _ = rows_for(eng, oracle, n, t, V.SEED + 4300, True)
    dE, dK, dKB = to_dev(E), to_dev(K), to_dev(KB)
    e0, k0 = dE[:, :1].contiguous(), dK[:, :1].contiguous()
    one, one_ok = eng.ris_lincomb(e0, k0)
    rt, rt_ok = eng.ris_roundtrip_mul(e0.reshape(n, 32), k0.reshape(n, 5))
    assert torch.equal(one, rt) and torch.equal(one_ok, rt_ok) and 0 < int((one_ok == 0).sum()) < n
    keys, keys_ok = eng.ris_lincomb(e0, torch.zeros_like(k0), dKB)
    assert torch.equal(keys_ok, one_ok)
    assert torch.equal(keys[keys_ok == 1], eng.ris_mul_base_compress(dKB)[keys_ok == 1]) and not bool(keys[keys_ok == 0].any())
    got, ok = eng.ris_lincomb(dE, dK, dKB)
    D, dok = eng.ris_decompress(dE.reshape(n * t, 32))
    dok = (dok.reshape(n, t) != 0).all(dim=1)
    comp = eng.ris_compress(eng.ed_add(eng.ed_lincomb(D.reshape(n, t, 20), dK), eng.ed_mul_base(dKB)))
    torch.cuda.synchronize()
    assert torch.equal(ok == 1, dok) and 0 < int((ok == 0).sum()) < n
    assert torch.equal(got[dok], comp[dok]) and not bool(got[~dok].any())


@pytest.mark.parametrize("slots", [7, 1])
def test_ring_under_contention(eng, oracle, slots):
    """ZC_RING_SLOTS in the single digits and 1: waves queue for their multi-unit slots, the bytes are those of the default
    ring, twice in a row (the ring state is reset per launch), and the other users of the shared ring on the same context
    are not disturbed."""
    n = 1 << 13
    cases = {}
    for t in (2, 7):
        E, K, KB, _ = rows_for(eng, oracle, n, t, V.SEED + 4400 + t, True)
        cases[t] = (E, K, KB, eng.ris_lincomb(E, K, KB))
    E1, K1 = np.ascontiguousarray(cases[2][0][:, 0]), np.ascontiguousarray(cases[2][1][:, 0])
    P2, _ = eng.ris_decompress(cases[2][0].reshape(2 * n, 32))
    P2 = P2.reshape(n, 2, 20)
    rt_ref, lc_ref = eng.ris_roundtrip_mul(E1, K1), eng.ed_lincomb(P2, cases[2][1])
    with V.tuned(ZC_RING_SLOTS=slots) as e:
        for t in (2, 7, 2):
            E, K, KB, ref = cases[t]
            RR.assert_same_bytes(e.ris_lincomb(E, K, KB), ref)
            RR.assert_same_bytes(e.ris_lincomb(E, K, KB), ref)
            RR.assert_same_bytes(e.ris_roundtrip_mul(E1, K1), rt_ref)
            assert np.array_equal(e.ed_lincomb(P2, cases[2][1]), lc_ref)
    for t in (2, 7):
        E, K, KB, ref = cases[t]
        RR.assert_same_bytes(ref, RR.oracle_ris_lincomb(oracle, E, K, KB))


def test_argument_errors(eng, oracle):
    lib, ctx = eng.lib, eng.ctx
    E, K, KB, _ = rows_for(eng, oracle, 512, 8, V.SEED + 4500, True)
    out = np.full((512, 32), 0xA5, dtype=np.uint8)
    ok = np.full(512, 0xA5, dtype=np.uint8)
    clean = lambda: bool((out == 0xA5).all() and (ok == 0xA5).all())
    e, k, kb, o, m = E.ctypes.data, K.ctypes.data, KB.ctypes.data, out.ctypes.data, ok.ctypes.data
    call = lambda *a: lib.zc_ris_lincomb(ctx, *a)
    assert call(e, k, 0, kb, o, m, 2) == ZC_ERR_BAD_ARG
    assert call(e, k, 9, None, o, m, 2) == ZC_ERR_BAD_ARG
    assert call(e, k, 8, kb, o, m, 2) == ZC_ERR_BAD_ARG                              # the base term would be a ninth scalar slot
    assert call(e, k, 2, kb, o, m, 1 << 30) == ZC_ERR_BAD_ARG                        # n * terms = 2^31
    assert call(None, k, 2, kb, o, m, 2) == ZC_ERR_BAD_ARG
    assert call(e, None, 2, kb, o, m, 2) == ZC_ERR_BAD_ARG
    assert call(e, k, 2, kb, None, m, 2) == ZC_ERR_BAD_ARG
    assert lib.zc_ris_lincomb(None, e, k, 2, kb, o, m, 2) == ZC_ERR_BAD_ARG
    assert call(e, k, 7, kb, o, m, 0) == ZC_OK and call(e, k, 8, None, o, m, 0) == ZC_OK
    assert clean()                                                                    # n == 0 and the failures above wrote nothing
    dK, dKB, dO = to_dev(K), to_dev(KB), to_dev(out)
    assert call(e, dK.data_ptr(), 7, kb, o, m, 2) == ZC_ERR_MIXED_MEM
    assert call(e, k, 7, dKB.data_ptr(), o, m, 2) == ZC_ERR_MIXED_MEM                # a device base array beside host arrays
    assert call(e, k, 7, kb, dO.data_ptr(), m, 2) == ZC_ERR_MIXED_MEM
    assert clean() and bool((dO == 0xA5).all())
    with pytest.raises(AssertionError):
        eng.ris_lincomb(E, K[:1])
    with pytest.raises(AssertionError):
        eng.ris_lincomb(E[:, :7], K[:, :7], KB[:1])
    empty = eng.ris_lincomb(E[:0], K[:0])
    assert empty[0].shape == (0, 32) and empty[1].shape == (0,)
    for t, base in ((8, None), (7, KB)):                                              # the context is as usable as before
        Et, Kt = np.ascontiguousarray(E[:, :t]), np.ascontiguousarray(K[:, :t])
        RR.assert_same_bytes(eng.ris_lincomb(Et, Kt, base), RR.oracle_ris_lincomb(oracle, Et, Kt, base))
