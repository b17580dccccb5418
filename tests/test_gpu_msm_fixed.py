"""GPU tier: the fixed-base MSM (zc_msm_bases_create / zc_msm_fixed / zc_msm_bases_destroy / zc_msm_fixed_plan).
Every sum is compared with the CPU oracle's sum of the reference's own Mul<Scalar> + Add on the same bases and ONE scalar
vector: the same group element (ed_eq) and the same compressed Edwards and Ristretto bytes."""
import ctypes as C

import numpy as np
import pytest

from tests import vectors as V

pytestmark = pytest.mark.gpu

ZC_ERR_BAD_ARG, ZC_ERR_MIXED_MEM = -1, -5


@pytest.fixture(scope="module")
def eng():
    import dusk_zerocaf_amd as z
    e = z.Engine()
    yield e
    e.close()


def same_point(oracle, got, want):
    got, want = np.asarray(got).reshape(1, 20), np.asarray(want).reshape(1, 20)
    assert oracle.ed_eq(got, want)[0] == 1
    assert np.array_equal(oracle.ed_compress(got)[0], oracle.ed_compress(want)[0])
    assert np.array_equal(oracle.ris_compress(got), oracle.ris_compress(want))


def bases(oracle, n, seed):
    """n subgroup points with one identity and some repeated bases."""
    small = V.base_multiples(oracle, min(n, 1 << 10), seed)
    P = np.tile(small, (n // len(small) + 1, 1))[:n].copy()
    if n >= 3:
        P[n // 2] = V.IDENT_ROW
        P[-1] = P[0]
    return P


def scalar_batch(n, batch, seed):
    """batch x n scalars: zero, one, all 260 bits, the raw >= 2^256 / early-stopping patterns, runs of equal scalars; the last
    vector of a batch > 1 is all zeros."""
    K = np.stack([V.rand_scalars_np(n, seed + b, bits=252) for b in range(batch)])
    edges = V.raw_scalar_edges(n_random=0)
    for b in range(batch):
        k = K[b]
        k[0] = 0
        if n > 1:
            k[1] = [1, 0, 0, 0, 0]
        if n > 2:
            k[2] = [(1 << 52) - 1] * 5
        if n > 3:
            e = edges[(b * 7) % len(edges):][: n - 3]
            k[3:3 + len(e)] = e
        if n >= 64:
            k[-20:] = k[-21]                                    # a long run of equal scalars
    if batch > 1:
        K[-1] = 0
    return K


@pytest.mark.parametrize("n", [1, 2, 3, 64, 257, 4096 + 13])
@pytest.mark.parametrize("batch", [1, 5])
def test_fixed_base_msm_vs_oracle(eng, oracle, n, batch):
    P = bases(oracle, n, V.SEED + 300 + n)
    K = scalar_batch(n, batch, V.SEED + 310 + n)
    with eng.msm_bases(P) as tb:
        got = tb.msm(K if batch > 1 else K[0])
    assert got.shape == (batch, 20)
    for b in range(batch):
        same_point(oracle, got[b], oracle.msm_naive(P, K[b]))
    if batch > 1:                                               # the all-zero vector: the identity
        assert oracle.ed_eq(got[-1:], np.array([V.IDENT_ROW], dtype=np.uint64))[0] == 1


def test_every_window_width(eng, oracle):
    n = (1 << 12) + 11
    P = bases(oracle, n, V.SEED + 320)
    K = scalar_batch(n, 1, V.SEED + 321)
    want = oracle.msm_naive_mt(P, K[0])
    for c in range(5, 23):
        plan = eng.msm_fixed_plan(n, c)
        assert plan["window_bits"] == c and plan["windows"] == -(-261 // c) and plan["record_stride"] == 128
        with eng.msm_bases(P, window_bits=c) as tb:
            assert tb.plan == plan
            got = tb.msm(K)
        same_point(oracle, got[0], want)


def test_table_reuse_interleaved_with_zc_msm(eng):
    n = 5000
    P = eng.ed_mul_base(V.rand_scalars_np(n, V.SEED + 330, bits=249))
    P[17] = V.IDENT_ROW
    with eng.msm_bases(P) as tb:
        for i, batch in enumerate((1, 3, 1)):
            K = scalar_batch(n, batch, V.SEED + 331 + 10 * i)
            want = [eng.msm(P, K[b]) for b in range(batch)]
            got = tb.msm(K)
            eng.msm(P[:4500], K[0][:4500])                     # a zc_msm between the fixed-base calls, other size
            for b in range(batch):
                assert eng.ed_eq(got[b:b + 1], want[b])[0] == 1


def test_2_20_bases_batch_2(eng, oracle):
    n = 1 << 20
    P = eng.ed_mul_base(V.rand_scalars_np(n, V.SEED + 340, bits=249))
    K = scalar_batch(n, 2, V.SEED + 341)
    K[1] = V.rand_scalars_np(n, V.SEED + 342, bits=252)
    with eng.msm_bases(P) as tb:
        assert tb.plan["window_bits"] >= 17
        got = tb.msm(K)
    for b in range(2):
        assert eng.ed_eq(got[b:b + 1], eng.msm(P, K[b]))[0] == 1
    same_point(oracle, got[0], oracle.msm_naive_mt(P, K[0]))


def test_device_scalars_and_residency(eng):
    import torch
    n = 3000
    P = eng.ed_mul_base(V.rand_scalars_np(n, V.SEED + 350, bits=249))
    K = scalar_batch(n, 3, V.SEED + 351)
    with eng.msm_bases(torch.from_numpy(P.view(np.int64)).cuda()) as tb:
        host = tb.msm(K)
        dev = tb.msm(torch.from_numpy(K.view(np.int64)).cuda())
        assert np.array_equal(host, dev)
        if torch.cuda.device_count() > 1:
            other = torch.from_numpy(K.view(np.int64)).to("cuda:1")
            assert eng.lib.zc_msm_fixed(eng.ctx, C.c_uint64(tb.id), other.data_ptr(), 3, host.ctypes.data) == ZC_ERR_MIXED_MEM


def test_lifecycle(oracle):
    import torch
    import dusk_zerocaf_amd as z
    P = bases(oracle, 100, V.SEED + 360)
    K = scalar_batch(100, 1, V.SEED + 361)
    out = np.empty((1, 20), dtype=np.uint64)
    a, b = z.Engine(), z.Engine()
    try:
        lib = a.lib
        ta, tb = a.msm_bases(P), b.msm_bases(P)
        assert ta.id != 0 and tb.id != 0 and ta.id != tb.id
        assert lib.zc_msm_fixed(a.ctx, C.c_uint64(tb.id), K.ctypes.data, 1, out.ctypes.data) == ZC_ERR_BAD_ARG   # another context's id
        assert lib.zc_msm_bases_destroy(a.ctx, C.c_uint64(tb.id)) == ZC_ERR_BAD_ARG
        assert lib.zc_msm_fixed(a.ctx, C.c_uint64(ta.id), K.ctypes.data, 0, None) == 0                          # batch 0: nothing to do
        dead = ta.id
        ta.close()
        assert lib.zc_msm_fixed(a.ctx, C.c_uint64(dead), K.ctypes.data, 1, out.ctypes.data) == ZC_ERR_BAD_ARG    # destroyed id
        assert lib.zc_msm_bases_destroy(a.ctx, C.c_uint64(dead)) == ZC_ERR_BAD_ARG                              # double destroy
        assert lib.zc_msm_bases_destroy(a.ctx, C.c_uint64(0)) == ZC_ERR_BAD_ARG
        a.msm_bases(P)                                          # left live: zc_ctx_destroy frees it
        assert lib.zc_ctx_destroy(a.ctx) == 0
        a.ctx = C.c_void_p()
        tb.id = 0
        assert lib.zc_ctx_destroy(b.ctx) == 0                   # with tb live
        b.ctx = C.c_void_p()
    finally:
        a.close()
        b.close()
    # create / destroy cycles leak nothing
    e = z.Engine()
    try:
        n = 1 << 18
        P = e.ed_mul_base(V.rand_scalars_np(n, V.SEED + 362, bits=249))
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        for _ in range(5):
            e.msm_bases(P).close()
        torch.cuda.synchronize()
        assert abs(torch.cuda.mem_get_info()[0] - free0) < (8 << 20)
    finally:
        e.close()


def test_bad_arguments(eng, oracle):
    lib, ctx = eng.lib, eng.ctx
    P = bases(oracle, 64, V.SEED + 370)
    ident = C.c_uint64(0)
    v = (C.c_int32 * 8)()
    for wb in (-1, 1, 4, 23, 64):
        assert lib.zc_msm_bases_create(ctx, P.ctypes.data, 64, wb, C.byref(ident)) == ZC_ERR_BAD_ARG
        assert lib.zc_msm_fixed_plan(ctx, 64, wb, v, 8) == ZC_ERR_BAD_ARG
    assert lib.zc_msm_bases_create(ctx, P.ctypes.data, 0, 0, C.byref(ident)) == ZC_ERR_BAD_ARG
    assert ident.value == 0
    # n W >= 2^31: refused by the plan query (and by create, before anything is allocated or read)
    for c in (5, 13, 22):
        W = -(-261 // c)
        lim = -(-(1 << 31) // W)
        assert lib.zc_msm_fixed_plan(ctx, lim, c, v, 8) == ZC_ERR_BAD_ARG
        assert lib.zc_msm_fixed_plan(ctx, lim - 1, c, v, 8) == 0 and v[0] == c and v[1] == W
        assert lib.zc_msm_bases_create(ctx, P.ctypes.data, lim, c, C.byref(ident)) == ZC_ERR_BAD_ARG
    assert lib.zc_msm_fixed_plan(ctx, 1 << 31, 0, v, 8) == ZC_ERR_BAD_ARG
    assert lib.zc_msm_fixed_plan(ctx, 64, 0, v, 7) == ZC_ERR_BAD_ARG
    # batch n W >= 2^32: refused before the scalars are read
    with eng.msm_bases(P, window_bits=22) as tb:
        W = tb.plan["windows"]
        big = -(-(1 << 32) // (64 * W))
        out = np.empty((1, 20), dtype=np.uint64)
        K = np.zeros((1, 64, 5), dtype=np.uint64)
        assert lib.zc_msm_fixed(ctx, C.c_uint64(tb.id), K.ctypes.data, big, out.ctypes.data) == ZC_ERR_BAD_ARG
        assert lib.zc_msm_fixed(ctx, C.c_uint64(tb.id), None, 1, out.ctypes.data) == ZC_ERR_BAD_ARG
    # the plan query reports what create uses
    for n in (1, 4107, 1 << 16, 1 << 20):
        plan = eng.msm_fixed_plan(n)
        assert 5 <= plan["window_bits"] <= 22 and plan["windows"] == -(-261 // plan["window_bits"])
    with eng.msm_bases(P) as tb:
        assert tb.plan == eng.msm_fixed_plan(64)
