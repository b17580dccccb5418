"""GPU tier: the reshaped generic step of k_ed_scalar_mul_pw (no early return for retired lanes, the result committed to Q or
N inside the branches) on tiles whose lanes add, double and retire at different steps.

2^17 + 77 rows, the smallest batch that takes the persistent kernel with a ragged last tile (13 lanes).  256 rows carry scalars
of ONE cost (bit length - 1 + popcount = 16) in every shape that cost has between 0x8000 (fifteen doublings, one addition)
and nine-bit scalars with eight bits set: the cost sort puts them next to each other, so whole tiles consist of lanes that
want an addition while their neighbours want a doubling, and that retire at different steps.  Zero scalars (lanes inactive
from the first step) fill the cheapest tile, and two off-curve points switch the doubling steps off for their tiles.
Every row must be the same under the default schedule and ZC_SCHED=unified, and a spread sample of 4096 rows plus every
special row the oracle's, limb for limb."""
import itertools

import numpy as np
import pytest

from oracle import pymodel as pm
from tests import vectors as V

pytestmark = pytest.mark.gpu

N = (1 << 17) + 77
COST = 16


def cost16_scalars(per_class=32):
    """Scalars with bit length b and popcount 17 - b, b = 9 .. 16: up to `per_class` distinct shapes each."""
    vals = []
    for b in range(9, 17):
        low = COST + 1 - b - 1                                          # set bits below the top bit
        shapes = itertools.islice(itertools.combinations(range(b - 1), low), 0, None, max(1, (b * b) // 40))
        for bits in itertools.islice(shapes, per_class):
            vals.append((1 << (b - 1)) | sum(1 << i for i in bits))
    assert all(v.bit_length() - 1 + bin(v).count("1") == COST for v in vals) and len(set(vals)) >= 100
    return vals


def test_mixed_tiles_default_equals_unified_and_the_oracle(oracle):
    rng = np.random.default_rng(V.SEED + 1800)
    with V.tuned() as eng:
        P = np.array(eng.ed_mul_base(V.rand_scalars_np(N, V.SEED + 1801, bits=249)), dtype=np.uint64)
        K = V.rand_scalars_np(N, V.SEED + 1802, bits=252)
        shapes = cost16_scalars()
        rows = rng.choice(N, size=256 + 40 + 2, replace=False)
        same_cost, zeros, off = rows[:256], rows[256:296], rows[296:]
        K[same_cost] = np.array([pm.limbs(shapes[i % len(shapes)]) for i in range(256)], dtype=np.uint64)
        K[zeros] = 0
        xy = V.limbs_array(V.rand_fe(40, V.SEED + 1803)[30:34])
        one = np.array(pm.limbs(1), dtype=np.uint64)
        P[off] = np.concatenate([xy[:2], xy[2:], np.tile(one, (2, 1)), oracle.fe_mul(xy[:2], xy[2:])], axis=1)   # T Z = X Y, off the curve
        K[off[0]] = pm.limbs(shapes[7])                                  # one among the equal-cost tiles, one under a random 252-bit scalar
        P[same_cost[5]] = V.IDENT_ROW
        got = np.asarray(eng.ed_scalar_mul(P, K))
    with V.tuned(ZC_SCHED="unified") as te:
        assert np.array_equal(got, np.asarray(te.ed_scalar_mul(P, K)))
    sample = np.unique(np.concatenate([np.linspace(0, N - 1, 4096).astype(np.int64), rows, np.arange(N - 13, N)]))
    assert len(sample) >= 4096
    assert np.array_equal(got[sample], oracle.mt(oracle.ed_scalar_mul, P[sample], K[sample]))
    assert (got[zeros] == np.array(V.IDENT_ROW, dtype=np.uint64)).all()
