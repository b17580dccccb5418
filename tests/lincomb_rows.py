"""Inputs and checks shared by the zc_ed_lincomb tests (CPU emulation tier and GPU tier).

The expected value is always composed from the oracle's own functions, in index order:
want = ((k0 P0 + k1 P1) + k2 P2) + ... with the reference's Mul<Scalar> and Add; a result passes when it is the same group
element (ed_eq) with the same compressed Edwards bytes / ok flags and the same Ristretto bytes -- on every row."""
import numpy as np

from oracle import pymodel as pm
from tests import vectors as V

BIT_LENGTHS = [4, 252, 60, 130, 17, 200, 1, 100]


def oracle_lincomb(oracle, P, K):
    """fold(ed_add, [ed_scalar_mul(P[:, j], K[:, j]) for j]) in index order, on all host cores."""
    t = P.shape[1]
    terms = [oracle.mt(oracle.ed_scalar_mul, np.ascontiguousarray(P[:, j]), np.ascontiguousarray(K[:, j])) for j in range(t)]
    acc = terms[0]
    for q in terms[1:]:
        acc = oracle.mt(oracle.ed_add, acc, q)
    return acc


def assert_same_points(oracle, got, want):
    got, want = np.ascontiguousarray(got, dtype=np.uint64), np.ascontiguousarray(want, dtype=np.uint64)
    assert got.shape == want.shape
    eq = oracle.mt(oracle.ed_eq, got, want)
    assert eq.all(), "rows that differ as group elements: %s" % np.flatnonzero(eq == 0)[:16]
    gb, gok = oracle.mt(oracle.ed_compress, got)
    wb, wok = oracle.mt(oracle.ed_compress, want)
    assert np.array_equal(gb, wb) and np.array_equal(gok, wok)
    assert np.array_equal(oracle.mt(oracle.ris_compress, got), oracle.mt(oracle.ris_compress, want))


def small_order_points(oracle):
    """The three non-trivial points of ed_coset4(identity)."""
    ident = np.array([V.IDENT_ROW], dtype=np.uint64)
    four = oracle.ed_coset4(ident).reshape(4, 20)
    keep = [r for r in four if oracle.ed_eq(r.reshape(1, 20), ident)[0] == 0]
    assert len(keep) == 3
    return np.array(keep, dtype=np.uint64)


def planted(oracle, t):
    """[(name, edit)]: edit(P_row (t, 20), K_row (t, 5)) rewrites one row in place."""
    rows = []

    def add(name):
        def deco(fn):
            rows.append((name, fn))
            return fn
        return deco

    @add("all scalars zero")
    def _(P, K): K[:] = 0

    @add("one term zero")
    def _(P, K): K[t // 2] = 0

    @add("scalar 1")
    def _(P, K): K[0] = [1, 0, 0, 0, 0]

    @add("all scalars 1")
    def _(P, K): K[:] = [1, 0, 0, 0, 0]

    @add("L")
    def _(P, K): K[t - 1] = pm.limbs(pm.L)

    @add("L - 1")
    def _(P, K): K[0] = pm.limbs(pm.L - 1)

    @add("all limbs 2^52 - 1")
    def _(P, K): K[t // 2] = [(1 << 52) - 1] * 5

    @add("all limbs 2^52 - 1 in every term")
    def _(P, K): K[:] = [(1 << 52) - 1] * 5

    for e, pat in enumerate(V.raw_scalar_edges()):
        def edge(P, K, e=e, pat=pat): K[e % t] = pat
        rows.append(("raw scalar edge %d" % e, edge))

    @add("identity point in one term")
    def _(P, K): P[t - 1] = V.IDENT_ROW

    @add("identity points in every term")
    def _(P, K): P[:] = V.IDENT_ROW

    @add("equal points")
    def _(P, K): P[:] = P[0]

    @add("equal points, equal scalars")
    def _(P, K):
        P[:] = P[0]
        K[:] = K[0]

    if t >= 2:
        @add("P1 = -P0, k1 = k0")
        def _(P, K):
            P[1] = oracle.ed_neg(P[0:1])[0]
            K[1] = K[0]
            K[2:] = 0

        @add("P1 = -P0, k1 = k0, the rest random")
        def _(P, K):
            P[1] = oracle.ed_neg(P[0:1])[0]
            K[1] = K[0]

    @add("very different bit lengths")
    def _(P, K):
        rng = np.random.default_rng(V.SEED + 77)
        for j in range(t):
            bits = BIT_LENGTHS[j]
            v = (int.from_bytes(rng.bytes(32), "little") % (1 << bits)) | (1 << (bits - 1))
            K[j] = pm.limbs(v)

    @add("short scalars only")
    def _(P, K): K[:, 1:] = 0

    small = small_order_points(oracle)
    for s in range(3):
        def torsion(P, K, s=s): P[s % t] = small[s]
        rows.append(("small-order point %d" % s, torsion))

    @add("small-order points in every term")
    def _(P, K):
        for j in range(t):
            P[j] = small[j % 3]
    return rows


def lincomb_rows(oracle, n, t, seed, points=None):
    """(P (n, t, 20), K (n, t, 5), positions of the planted rows): valid subgroup points in non-trivial extended coordinates,
    252-bit scalars, and every family of planted() written over rows 3, 10, 17, ... (several waves).
    points(count, seed) -> (count, 20) supplies the points (default: the oracle's r_i * B on all host cores)."""
    if points is None:
        def points(count, s):
            k = V.rand_scalars_np(count, s, bits=249)
            b = np.tile(np.array(sum(pm.pt_limbs(pm.BASEPOINT), []), dtype=np.uint64), (count, 1))
            return oracle.mt(oracle.ed_scalar_mul, b, k)
    P = np.array(points(n * t, seed), dtype=np.uint64).reshape(n, t, 20)
    K = V.rand_scalars_np(n * t, seed + 1, bits=252).reshape(n, t, 5)
    where = []
    for idx, (_, edit) in enumerate(planted(oracle, t)):
        pos = 3 + 7 * idx
        assert pos < n, "batch too small for the planted rows"
        edit(P[pos], K[pos])
        where.append(pos)
    return P, K, where
