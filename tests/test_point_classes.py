"""CPU tier: the point catalogue of tests/point_classes.py is what it claims to be, and the independent big-integer model
(oracle/pymodel.py) agrees with the C oracle on every class -- so the expectations the GPU tier takes from the oracle on
torsion and mixed-order points are themselves checked on a machine without a GPU."""
import numpy as np
import pytest

from oracle import pymodel as pm
from tests import point_classes as PC
from tests import vectors as V

N = 64
SEED = V.SEED + 0x7050


def ints(row):
    return tuple(pm.from_limbs(row[5 * c:5 * c + 5]) for c in range(4))


def rows_of(pts):
    return np.array([sum(pm.pt_limbs(p), []) for p in pts], dtype=np.uint64)


@pytest.fixture(scope="module")
def catalogue(oracle):
    return PC.classes(oracle, N, SEED)


def test_torsion_rows(oracle):
    T = PC.torsion(oracle)
    assert T.shape == (8, 20)
    assert [PC.order_in_e8(oracle, r) for r in T] == [1, 8, 4, 8, 2, 8, 4, 8]
    assert ints(T[0]) == pm.IDENT and ints(T[4]) == (0, pm.P - 1, 1, 0)
    # the group law on the rows is addition of indices mod 8, in the model too
    for i in range(8):
        for j in range(8):
            assert pm.ed_eq(pm.ed_add(ints(T[i]), ints(T[j])), ints(T[(i + j) % 8])), (i, j)
    assert pm.L % 8 == 3
    # the y = 0 points are the two of order 4, the x = 0 points the identity and (0, -1)
    assert [j for j in range(8) if ints(T[j])[1] == 0] == [2, 6] and [j for j in range(8) if ints(T[j])[0] == 0] == [0, 4]
    assert np.array_equal(PC.torsion_index(oracle, T[::-1]), np.arange(8)[::-1])


def test_classes_are_what_they_claim(oracle, catalogue):
    assert set(catalogue) == set(PC.CLASS_NAMES) | {"scaled"}
    T = PC.torsion(oracle)
    Lmul = {name: PC.times_L(oracle, rows) for name, rows in catalogue.items()}
    assert PC.is_identity(oracle, Lmul["subgroup"]).all()
    assert np.array_equal(PC.torsion_index(oracle, Lmul["torsion"]), 3 * (np.arange(N) % 8) % 8)
    for name, order in (("order_2L", 2), ("order_4L", 4), ("order_8L", 8)):
        assert {PC.order_in_e8(oracle, r) for r in Lmul[name]} == {order}
    assert len({PC.order_in_e8(oracle, r) for r in Lmul["decoded"]}) >= 3
    # scaled: the same group elements in other coordinates, Z != 1, all six classes present
    org = PC.scaled_origin(N)
    assert {name for name, _ in org} == set(PC.CLASS_NAMES)
    for i, (name, j) in enumerate(org):
        assert pm.ed_eq(ints(catalogue["scaled"][i]), ints(catalogue[name][j]))
        assert ints(catalogue["scaled"][i])[2] != 1
    lam = [ints(r) for r in catalogue["scaled"] if ints(r)[0] == 0]
    assert any(y == z for _, y, z, _ in lam) and any((y + z) % pm.P == 0 for _, y, z, _ in lam)   # (0, l, l, 0) and (0, -l, l, 0)
    # the even-subgroup map the GPU tier asserts zc_ris_is_valid against is the oracle's own answer
    want = PC.in_even_subgroup(oracle, catalogue)
    assert set(want) == set(catalogue)
    for name in want:
        assert np.array_equal(oracle.mt(oracle.ris_is_valid, catalogue[name]) == 1, want[name]), name
    assert want["subgroup"].all() and want["torsion"].sum() == N // 8 and not want["order_8L"].any() and 0 < want["scaled"].sum() < N
    for name, rows in catalogue.items():
        assert oracle.ed_is_valid(rows).all(), name
        for r in rows:                                                                              # the curve equation and T Z = X Y
            x, y, z, t = ints(r)
            assert (-x * x + y * y) * z * z % pm.P == (z ** 4 + pm.D * x * x * y * y) % pm.P and (t * z - x * y) % pm.P == 0


def test_scalars_for_torsion():
    K = PC.scalars_for_torsion()
    vals = [pm.from_limbs(k) for k in K]
    for v in PC.edge_scalars() + [sum(PC.M52 << (52 * i) for i in range(5))]:
        assert v in vals
    assert (K <= PC.M52).all() and len(K) == 15 + len(V.raw_scalar_edges())
    # L, 2L, 4L and 8L +- 1 are where "right mod L" and "right as an integer" part on a point of order 8L
    assert [v % 8 for v in (pm.L, 2 * pm.L, 4 * pm.L)] == [3, 6, 4] and (8 * pm.L + 1) % pm.L == 1
    # effective_scalar: the identity below 2^256, the early stop of the raw edges above (V.raw_scalar_edges's own examples)
    assert all(PC.effective_scalar(v) == v for v in PC.edge_scalars())
    assert [PC.effective_scalar(pm.from_limbs(k)) for k in ([0, 0, 0, 0, 1 << 50], [1, 0, 0, 0, 1 << 50], [7, 0, 0, 0, 8 << 48])] == [0, 1, 7]
    assert PC.effective_scalar(pm.from_limbs([8, 0, 0, 0, 8 << 48])) == pm.from_limbs([8, 0, 0, 0, 8 << 48])

def test_model_agrees_with_oracle_on_every_class(oracle, catalogue):
    """ed_scalar_mul (every limb), ed_add, ed_compress and ris_compress: pymodel against the C oracle on every class."""
    E = PC.scalars_for_torsion()
    for c, (name, P) in enumerate(catalogue.items()):
        K = V.rand_scalars_np(N, SEED + 100 + c, bits=252)
        K[:len(E)] = np.roll(E, c, axis=0)[:N]
        pts = [ints(r) for r in P]
        got = oracle.mt(oracle.ed_scalar_mul, P, K)
        want = [pm.ed_scalar_mul(p, pm.from_limbs(k)) for p, k in zip(pts, K)]
        assert np.array_equal(got, rows_of(want)), name
        if name == "torsion":                                                                       # the closed form on E[8]
            j = (np.arange(N) % 8).tolist()
            eff = [PC.effective_scalar(pm.from_limbs(k)) for k in K]
            assert np.array_equal(PC.torsion_index(oracle, got), np.array([e * i % 8 for e, i in zip(eff, j)]))
        Q =np.roll(catalogue["order_8L"], c + 1, axis=0)
        for other, what in ((Q, "Q"), (P, "P + P"), (oracle.ed_neg(P), "P - P")):
            assert np.array_equal(oracle.ed_add(P, other), rows_of([pm.ed_add(p, ints(q)) for p, q in zip(pts, other)])), (name, what)
        for rows, mp in ((P, pts), (got, want)):
            live = [i for i, p in enumerate(mp) if p[2] % pm.P]
            assert len(live) == N
            cb, ok = oracle.ed_compress(rows)
            assert ok.all() and [bytes(b.tolist()) for b in cb] == [pm.ed_compress(p) for p in mp], name
            assert [bytes(b.tolist()) for b in oracle.ris_compress(rows)] == [pm.ris_compress(p) for p in mp], name
