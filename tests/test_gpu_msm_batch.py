"""GPU tier: the batched variable-base MSM (zc_msm_batch / zc_msm_batch_plan).  Every instance's sum is compared with the CPU
oracle's sum of the reference's own Mul<Scalar> + Add over that instance's rows: the same group element (ed_eq) and the same
compressed Edwards and Ristretto bytes.  Both regimes run: strict scalar multiplications + a fold per instance below the
crossover, one bucket pipeline over all instances from it on."""
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


@pytest.fixture(scope="module")
def crossover(eng):
    """The smallest n the library takes the bucket regime for (at batch 2; the regime depends on n only)."""
    regimes = [eng.msm_batch_plan(n, 2)["regime"] for n in range(1, (1 << 14) + 1)]
    assert regimes[-1] == "buckets" and regimes[0] == "scalar_mul"
    x = regimes.index("buckets") + 1
    assert all(r == "buckets" for r in regimes[x - 1:]) and all(r == "scalar_mul" for r in regimes[:x - 1])
    return x


def same_point(oracle, got, want):
    got, want = np.asarray(got).reshape(1, 20), np.asarray(want).reshape(1, 20)
    assert oracle.ed_eq(got, want)[0] == 1
    assert np.array_equal(oracle.ed_compress(got)[0], oracle.ed_compress(want)[0])
    assert np.array_equal(oracle.ris_compress(got), oracle.ris_compress(want))


def batch_points(eng, n, batch, seed):
    """batch x n subgroup points (k B on the device); identities and repeated points in some instances."""
    P = eng.ed_mul_base(V.rand_scalars_np(n * batch, seed, bits=249)).reshape(batch, n, 20)
    for b in range(batch):
        if n >= 3 and b % 2 == 0:
            P[b, n // 2] = V.IDENT_ROW
            P[b, -1] = P[b, 0]
        if b == 1:
            P[b, :] = P[b, 0]                                   # one instance over a single repeated point
    return P


def batch_scalars(n, batch, seed):
    """batch x n scalars: zeros, one, all 260 bits, raw >= 2^256 / early-stopping patterns, runs of equal scalars; one
    instance (the last of a batch > 1) all zeros."""
    K = V.rand_scalars_np(n * batch, seed, bits=252).reshape(batch, n, 5)
    edges = V.raw_scalar_edges(n_random=0)
    for b in range(batch):
        k = K[b]
        k[0] = 0
        if n > 1:
            k[1] = [1, 0, 0, 0, 0]
        if n > 2:
            k[2] = [(1 << 52) - 1] * 5
        if n > 3:
            e = edges[(b * 5) % len(edges):][: n - 3]
            k[3:3 + len(e)] = e
        if n >= 64:
            k[-24:] = k[-25]                                    # a run of equal scalars: one skewed bucket per window
    if batch > 1:
        K[-1] = 0
    return K


def check_vs_oracle(oracle, got, P, K, rows):
    for b in rows:
        same_point(oracle, got[b], oracle.msm_naive_mt(P[b], K[b]))


SHAPES = [(n, batch) for n in ("1", "2", "3", "X-1", "X", "4096") for batch in (1, 2, 7, 64)] + [("16384", b) for b in (1, 2, 7)]


@pytest.mark.parametrize("n_name,batch", SHAPES)
def test_batch_vs_oracle(eng, oracle, crossover, n_name, batch):
    n = {"X-1": crossover - 1, "X": crossover}.get(n_name) or int(n_name)
    P = batch_points(eng, n, batch, V.SEED + 400 + n + batch)
    K = batch_scalars(n, batch, V.SEED + 410 + n + batch)
    got = eng.msm_batch(P, K)
    assert got.shape == (batch, 20)
    plan = eng.msm_batch_plan(n, batch)
    if batch > 1:
        assert plan["regime"] == ("buckets" if n >= crossover else "scalar_mul")
        if n * batch >= 1 << 17:
            assert plan["affine"]                               # the shared affine normalisation ran
    check_vs_oracle(oracle, got, P, K, range(batch))
    if batch > 1:                                               # the all-zero instance: the identity
        assert oracle.ed_eq(got[-1:], np.array([V.IDENT_ROW], dtype=np.uint64))[0] == 1


def test_many_two_term_instances(eng, oracle):
    """2^16 instances of two pairs (Schnorr-style checks): every one against the device's own k P + k' P', a seeded
    subset against the oracle."""
    batch = 1 << 16
    P = batch_points(eng, 2, batch, V.SEED + 420)
    K = batch_scalars(2, batch, V.SEED + 421)
    got = eng.msm_batch(P, K)
    terms = eng.ed_scalar_mul(P.reshape(-1, 20), K.reshape(-1, 5)).reshape(batch, 2, 20)
    want = eng.ed_add(terms[:, 0], terms[:, 1])
    assert eng.ed_eq(got, want).all()
    rows = np.random.default_rng(V.SEED + 422).choice(batch, 24, replace=False)
    check_vs_oracle(oracle, got, P, K, list(rows) + [batch - 1])


def test_large_batch_vs_zc_msm(eng, oracle):
    """2^16 instances of 16 pairs and 64 of 2^12 + 5: every instance against zc_msm on its rows, a seeded subset against the
    oracle."""
    for n, batch, seed in ((16, 1 << 16, 430), (4096 + 5, 64, 440)):
        P = batch_points(eng, n, batch, V.SEED + seed)
        K = batch_scalars(n, batch, V.SEED + seed + 1)
        got = eng.msm_batch(P, K)
        want = np.concatenate([eng.msm(P[b], K[b]) for b in range(batch)])
        assert eng.ed_eq(got, want).all(), (n, batch)
        rows = np.random.default_rng(V.SEED + seed + 2).choice(batch, 4, replace=False)
        check_vs_oracle(oracle, got, P, K, rows)


def test_projective_records_and_device_inputs(eng, oracle):
    """Device-resident torch inputs give the host call's limbs; points that are not 16-byte aligned take the projective
    records even where batch n >= 2^17 would normalise to affine ones."""
    import torch
    n, batch = 4096, 40
    assert eng.msm_batch_plan(n, batch)["affine"] and not eng.msm_batch_plan(n, batch, points_aligned16=False)["affine"]
    P = batch_points(eng, n, batch, V.SEED + 450)
    K = batch_scalars(n, batch, V.SEED + 451)
    host = eng.msm_batch(P, K)
    dK = torch.from_numpy(K.view(np.int64)).cuda()
    dev = eng.msm_batch(torch.from_numpy(P.view(np.int64)).cuda(), dK)
    assert np.array_equal(host, dev)
    flat = torch.zeros(P.size + 2, dtype=torch.int64, device="cuda")
    flat[1:1 + P.size] = torch.from_numpy(P.reshape(-1).view(np.int64)).cuda()
    odd = flat[1:1 + P.size].view(batch, n, 20)                # 8 bytes past an aligned allocation
    assert odd.data_ptr() % 16 == 8
    unaligned = eng.msm_batch(odd, dK)
    assert eng.ed_eq(unaligned, host).all()
    check_vs_oracle(oracle, unaligned, P, K, [0, 1, batch - 1])
    # host points with device scalars: mixed residency
    out = np.empty((batch, 20), dtype=np.uint64)
    assert eng.lib.zc_msm_batch(eng.ctx, P.ctypes.data, dK.data_ptr(), n, batch, out.ctypes.data) == ZC_ERR_MIXED_MEM
    if torch.cuda.device_count() > 1:
        other = dK.to("cuda:1")
        dP = torch.from_numpy(P.view(np.int64)).cuda()
        assert eng.lib.zc_msm_batch(eng.ctx, dP.data_ptr(), other.data_ptr(), n, batch, out.ctypes.data) == ZC_ERR_MIXED_MEM


def test_empty_shapes(eng):
    lib, ctx = eng.lib, eng.ctx
    P = np.zeros((3, 1, 20), dtype=np.uint64)
    K = np.zeros((3, 1, 5), dtype=np.uint64)
    out = np.full((3, 20), 7, dtype=np.uint64)
    assert lib.zc_msm_batch(ctx, P.ctypes.data, K.ctypes.data, 0, 3, out.ctypes.data) == 0
    assert (out == np.array(V.IDENT_ROW, dtype=np.uint64)).all()
    out[:] = 7
    assert lib.zc_msm_batch(ctx, P.ctypes.data, K.ctypes.data, 5, 0, out.ctypes.data) == 0
    assert (out == 7).all()
    assert lib.zc_msm_batch(ctx, None, None, 5, 0, None) == 0
    assert eng.msm_batch(np.zeros((4, 0, 20), np.uint64), np.zeros((4, 0, 5), np.uint64)).tolist() == [V.IDENT_ROW] * 4


def test_limits(eng):
    """Every index limit gives ZC_ERR_BAD_ARG from the call and from the plan query, before anything is allocated or read
    (the small arrays passed here are far shorter than the shapes claimed)."""
    lib, ctx = eng.lib, eng.ctx
    P = np.zeros((1, 20), dtype=np.uint64)
    K = np.zeros((1, 5), dtype=np.uint64)
    out = np.zeros((1, 20), dtype=np.uint64)
    v = (C.c_int32 * 8)()

    def refused(n, batch):
        return (lib.zc_msm_batch(ctx, P.ctypes.data, K.ctypes.data, n, batch, out.ctypes.data) == ZC_ERR_BAD_ARG
                and lib.zc_msm_batch_plan(ctx, n, batch, 1, v, 8) == ZC_ERR_BAD_ARG)

    def accepted_by_plan(n, batch):
        return lib.zc_msm_batch_plan(ctx, n, batch, 1, v, 8) == 0

    def cw(n):
        assert accepted_by_plan(n, 2)
        return v[1], v[2]

    # record indices: batch n < 2^31
    assert refused(1, 1 << 31) and refused(1 << 16, 1 << 15) and refused(1 << 31, 1)
    assert accepted_by_plan(1 << 12, 1 << 10)
    # pair indices: batch n W < 2^32 with batch n < 2^31
    n = 1 << 12
    c, W = cw(n)
    lim = -(-(1 << 32) // (n * W))
    assert lim * n < 1 << 31 and refused(n, lim) and accepted_by_plan(n, lim - 1)
    # bucket keys: batch W 2^(c-1) < 2^32 with the other two limits met (n = 1: c = 5, W = 53)
    c, W = cw(1)
    lim = -(-(1 << 32) // (W << (c - 1)))
    assert lim * W < 1 << 32 and refused(1, lim) and accepted_by_plan(1, lim - 1)
    assert out.tolist() == [[0] * 20]                           # nothing was written
    assert lib.zc_msm_batch_plan(ctx, 64, 2, 1, v, 7) == ZC_ERR_BAD_ARG
    assert lib.zc_msm_batch(ctx, None, K.ctypes.data, 1, 1, out.ctypes.data) == ZC_ERR_BAD_ARG


def test_deterministic_and_interleaved(eng, oracle, crossover):
    """Two calls on the same inputs give the same limbs; zc_msm, zc_msm_batch, zc_msm_fixed, zc_msm_batch in a row all stay
    correct (they share the device's MSM workspace)."""
    for n, batch in ((4096, 9), (max(crossover - 1, 1), 33), (crossover, 33)):
        P = batch_points(eng, n, batch, V.SEED + 460 + n)
        K = batch_scalars(n, batch, V.SEED + 461 + n)
        a = eng.msm_batch(P, K)
        b = eng.msm_batch(P, K)
        assert np.array_equal(a, b), (n, batch)
    n, batch = 5000, 6
    P = batch_points(eng, n, batch, V.SEED + 470)
    K = batch_scalars(n, batch, V.SEED + 471)
    Q = batch_points(eng, 300, 4, V.SEED + 472)
    L = batch_scalars(300, 4, V.SEED + 473)
    want = [eng.msm(P[b], K[b]) for b in range(batch)]
    with eng.msm_bases(P[0]) as tb:
        for _ in range(2):
            m = eng.msm(P[2], K[2])
            got = eng.msm_batch(P, K)
            fx = tb.msm(K[:3])
            got2 = eng.msm_batch(Q, L)
            assert eng.ed_eq(m, want[2])[0] == 1
            assert all(eng.ed_eq(got[b:b + 1], want[b])[0] == 1 for b in range(batch))
            assert eng.ed_eq(fx[0:1], want[0])[0] == 1
            check_vs_oracle(oracle, got2, Q, L, range(4))


def test_one_workspace_serves_every_pipeline(oracle):
    """zc_msm, zc_msm_batch and zc_msm_fixed lay their buffers out in ONE device allocation, each from its own plan.  On a
    fresh context, in this order: the smallest bucket-regime shape of each (4096 pairs; 3 instances of 64; 2 vectors over 64
    bases), a zc_msm of 8192 + 5 pairs, which needs more than the allocation holds and so replaces it, then the first three
    again.  Every sum is the oracle's group element, every repeat has the limbs of its first run."""
    import dusk_zerocaf_amd as z
    e = z.Engine()
    try:
        big = 8192 + 5
        P = batch_points(e, big, 1, V.SEED + 480)[0]
        K = batch_scalars(big, 1, V.SEED + 481)[0]
        Pb = batch_points(e, 64, 3, V.SEED + 482)
        Kb = batch_scalars(64, 3, V.SEED + 483)
        Kf = batch_scalars(64, 2, V.SEED + 484)
        assert e.msm_plan(4096)["window_bits"] and not e.msm_plan(4095)["window_bits"]
        assert e.msm_batch_plan(64, 3)["regime"] == "buckets" and e.msm_batch_plan(63, 3)["regime"] == "scalar_mul"
        with e.msm_bases(Pb[0]) as tb:
            def three():
                return e.msm(P[:4096], K[:4096]), e.msm_batch(Pb, Kb), tb.msm(Kf)
            m1, b1, f1 = three()
            g = e.msm(P, K)
            m2, b2, f2 = three()
        same_point(oracle, m1, oracle.msm_naive_mt(P[:4096], K[:4096]))
        check_vs_oracle(oracle, b1, Pb, Kb, range(3))
        for v in range(2):
            same_point(oracle, f1[v], oracle.msm_naive_mt(Pb[0], Kf[v]))
        same_point(oracle, g, oracle.msm_naive_mt(P, K))
        assert np.array_equal(m1, m2) and np.array_equal(b1, b2) and np.array_equal(f1, f2)
    finally:
        e.close()
