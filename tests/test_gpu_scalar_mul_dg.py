"""GPU tier: the persistent strict scalar-mul kernel on its doubling/generic schedule (k_ed_scalar_mul_pw: generic steps
alternating with wave-uniform 3S+5M doubling steps, one stashed addend per lane) and the unified-step kernel kept behind
ZC_SCHED=unified -- every (X:Y:Z:T) limb against the oracle's double_and_add, with the edge scalars and the four kinds of
invalid rows scattered through the batch so that both all-valid tiles (doubling steps) and fallback tiles (a lane fails the
validity gate: generic steps only) occur; host and device-resident inputs; and default == unified on bench.py's inputs."""
import numpy as np
import pytest

from oracle import pymodel as pm
from tests import vectors as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import dusk_zerocaf_amd as z
    e = z.Engine()
    yield e
    e.close()


def eq(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def scatter_edges(oracle, P, K, seed):
    """Edge scalars and invalid points at seeded random rows (the cost sort then spreads them over the tiles)."""
    n = len(P)
    rng = np.random.default_rng(seed)
    scal = [[0] * 5, [1, 0, 0, 0, 0], pm.limbs(pm.L), pm.limbs(pm.L - 1), pm.limbs(2**249 - 1), [(1 << 52) - 1] * 5,
            [0, 0, 0, 0, 1 << 47], pm.limbs(8), pm.limbs(2**248), pm.limbs((1 << 252) - 1)]
    scal = np.concatenate([np.array(scal, dtype=np.uint64), V.raw_scalar_edges(n_random=40)])
    rows = rng.choice(n, size=3 * len(scal) + 4 * 40 + 8, replace=False)
    srows, prows = rows[:3 * len(scal)], rows[3 * len(scal):]
    K[srows] = np.tile(scal, (3, 1))
    off, badt, z0, big, ident = [prows[40 * i:40 * i + 40] for i in range(4)] + [prows[160:]]
    xy = V.limbs_array(V.rand_fe(200, seed + 1)[40:120])
    one = np.array(pm.limbs(1), dtype=np.uint64)
    P[off] = np.concatenate([xy[:40], xy[40:], np.tile(one, (40, 1)), oracle.fe_mul(xy[:40], xy[40:])], axis=1)   # T Z = X Y, off the curve
    P[badt, 15:20] = oracle.fe_neg(P[badt, 15:20])                                     # on the curve, T Z = -X Y
    P[z0, 10:15] = 0
    P[z0[:4]] = 0                                                                      # the all-zero row (passes the gate)
    for r in big:                                                                      # limbs >= p: every coordinate + p
        P[r] = sum([pm.limbs(pm.from_limbs(P[r, 5 * c:5 * c + 5]) + pm.P) for c in range(4)], [])
    P[ident] = V.IDENT_ROW
    K[off[0]] = K[badt[0]] = pm.limbs((1 << 252) - 1)                                  # invalid rows under dense and sparse scalars too
    K[off[1]] = K[badt[1]] = pm.limbs(1 << 251)
    return P, K


@pytest.mark.parametrize("n", [(1 << 17) + 333, 1 << 20])
def test_dg_and_unified_schedules_every_limb_vs_oracle(eng, oracle, n):
    import torch
    P = np.array(eng.ed_mul_base(V.rand_scalars_np(n, V.SEED + 1700 + (n & 1), bits=249)), dtype=np.uint64)
    K = V.rand_scalars_np(n, V.SEED + 1702 + (n & 1), bits=252)
    P, K = scatter_edges(oracle, P, K, V.SEED + 1704)
    want = oracle.mt(oracle.ed_scalar_mul, P, K)
    for sched in (None, "unified"):
        with V.tuned(ZC_SCHED=sched) as te:
            assert eq(te.ed_scalar_mul(P, K), want), sched                              # host inputs
            dP, dK = (torch.from_numpy(a.view(np.int64)).cuda() for a in (P, K))
            got = te.ed_scalar_mul(dP, dK)                                              # device-resident inputs
            torch.cuda.synchronize()
            assert eq(got.cpu().numpy().view(np.uint64), want), sched


def test_default_equals_unified_on_the_benchmark_inputs(eng):
    """bench.py's headline inputs (make_inputs, seed 0x5EED0003, 2^20 units): the two schedules agree on every limb."""
    n = 1 << 20
    rng = np.random.default_rng(0x5EED0003)

    def scalars(bits):
        k = rng.integers(0, 1 << 52, size=(n, 5), dtype=np.uint64)
        k[:, 4] = rng.integers(0, 1 << (bits - 208), size=n, dtype=np.uint64)
        return k

    P = eng.ed_mul_base(scalars(249))
    K = scalars(252)
    got = eng.ed_scalar_mul(P, K)
    with V.tuned(ZC_SCHED="unified") as te:
        assert eq(got, te.ed_scalar_mul(P, K))
