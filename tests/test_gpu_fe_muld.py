"""GPU tier: every strict kernel that multiplies T by the curve constant d through fp_mul_d (d x = x/126297 - x, zc_curve.hip.h),
every limb against the oracle.  The routine is per lane, so the sizes only have to reach each kernel: the quad path (which
keeps d as a multiplier operand: the control), the block kernel, the small / independent-chain kernel, the persistent waves
on the default and on the unified schedule, the element-wise addition per lane and staged, and the broadcast doublings.
Identity, E[8] (T = 0 on the identity and the 2-torsion point), Z = 0, all-zero and limbs-above-p rows and the edge scalars
of tests/test_gpu_scalar_mul_dg.py stand in every batch; the oracle runs once on the largest batch and the smaller ones are
its first rows."""
import numpy as np
import pytest

from tests import point_classes as PC
from tests import vectors as V
from tests.test_gpu_scalar_mul_dg import scatter_edges

pytestmark = pytest.mark.gpu
N = (1 << 17) + 77
SEED = V.SEED + 0xD17


@pytest.fixture(scope="module")
def eng():
    import dusk_zerocaf_amd as z
    e = z.Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def batch(eng, oracle):
    """(P, K, oracle's K * P) of N rows.  The edge rows and as many ordinary ones, shuffled, come first, so that every prefix
    from 257 rows on holds edge rows of every kind next to ordinary ones; the rest follows in its order."""
    P0 = np.array(eng.ed_mul_base(V.rand_scalars_np(N, SEED, bits=249)), dtype=np.uint64)
    K0 = V.rand_scalars_np(N, SEED + 1, bits=252)
    P, K = scatter_edges(oracle, P0.copy(), K0.copy(), SEED + 2)
    rng = np.random.default_rng(SEED + 3)
    free = np.nonzero(~((P != P0).any(axis=1) | (K != K0).any(axis=1)))[0]
    tors = PC.torsion(oracle)
    trows = rng.choice(free, size=32, replace=False)
    P[trows] = tors[np.arange(32) % 8]                                                  # E[8], four times: random scalars
    K[trows[:8]] = np.array(PC.scalar_rows((1 << 252) - 1, 8))                          # and the densest one
    edge = np.nonzero((P != P0).any(axis=1) | (K != K0).any(axis=1))[0]
    assert 300 < len(edge) < 2000
    rest = np.setdiff1d(np.arange(N), edge)
    head = rng.permutation(np.concatenate([edge, rest[:len(edge)]]))
    order = np.concatenate([head, rest[len(edge):]])
    j = int(np.nonzero(order == trows[0])[0][0])
    order[[0, j]] = order[[j, 0]]                                                       # n = 1: the identity of E[8] under the dense scalar
    P, K = np.ascontiguousarray(P[order]), np.ascontiguousarray(K[order])
    kinds = edge_kinds(P[:257])
    assert all(kinds.values()), kinds
    return P, K, oracle.mt(oracle.ed_scalar_mul, P, K)


def edge_kinds(P):
    from oracle import pymodel as pm
    top = np.uint64(pm.P >> 208)
    return {"identity": (P == np.array(V.IDENT_ROW, dtype=np.uint64)).all(axis=1).any(), "all-zero": (~P.any(axis=1)).any(),
            "Z = 0": ((~P[:, 10:15].any(axis=1)) & P[:, 5:10].any(axis=1)).any(), "T = 0": ((~P[:, 15:20].any(axis=1)) & P[:, 10:15].any(axis=1)).any(),
            "limbs >= p": (P[:, 4] >= top).any()}


def eq(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize("n,sched", [(1, None), (257, None), ((1 << 14) + 1, None), (1 << 16, None), (N, None), (N, "unified")],
                         ids=["quad-1", "quad-257", "block", "small", "persistent", "persistent-unified"])
def test_scalar_mul_every_limb(batch, n, sched):
    P, K, want = batch
    with V.tuned(ZC_SCHED=sched) as te:
        assert eq(te.ed_scalar_mul(P[:n], K[:n]), want[:n])


@pytest.mark.parametrize("n", [257, 4397], ids=["per-lane", "staged"])
def test_ed_add_every_limb(eng, oracle, batch, n):
    P = batch[0]
    for shift in (1, 0, 7):                                                            # neighbours, P + P, another pairing
        Q = np.ascontiguousarray(np.roll(P[:n], shift, axis=0))
        assert eq(eng.ed_add(P[:n], Q), oracle.mt(oracle.ed_add, np.ascontiguousarray(P[:n]), Q)), shift


def test_mul_by_pow_2_every_limb(eng, oracle, batch):
    P = np.ascontiguousarray(batch[0][:300])
    for kexp in (1, 5, 249):
        assert eq(eng.ed_mul_by_pow_2(P, kexp), oracle.ed_mul_by_pow_2(P, kexp)), kexp
