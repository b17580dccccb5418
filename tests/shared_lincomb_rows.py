"""Rows, scalar vectors and expected results for the tests of zc_ed_lincomb_shared and zc_ris_lincomb_shared (CPU emulation and GPU
tier).  Rows are combinations of the pools of tests/shared_scalar_rows (at most 331 distinct rows, repeated for longer batches)
with planted rows in front; the oracle's answers are composed by tests/lincomb_rows and tests/ris_lincomb_rows from the
reference's own Mul<Scalar>, Add and codecs with the scalar vector tiled into every row, and cached per pool and vector."""
import random

import numpy as np

from oracle import pymodel as pm
from tests import lincomb_rows as R
from tests import ris_lincomb_rows as RR
from tests import shared_scalar_rows as S
from tests import vectors as V

SEED = S.SEED + 0x11C
NEG_ROWS, SAME_ROWS, IDENT_ROWS = range(0, 8), range(8, 16), range(16, 20)       # where the planted rows lie (t >= 2 for the first two)

_cache = {}


def point_rows(oracle, t):
    """(m, t, 20): term j of row i is pool[(i + 37 j) mod m] -- every class of tests/point_classes meets every other -- with
    P_i1 = -P_i0 in rows 0..7, P_i1 = P_i0 in rows 8..15 and every point the identity in rows 16..19."""
    key = ("P", t)
    if key not in _cache:
        pool, _ = S.point_pool(oracle)
        m = len(pool)
        P = np.stack([pool[(np.arange(m) + 37 * j) % m] for j in range(t)], axis=1).copy()
        if t >= 2:
            P[NEG_ROWS, 1] = oracle.ed_neg(np.ascontiguousarray(P[NEG_ROWS, 0]))
            P[SAME_ROWS, 1] = P[SAME_ROWS, 0]
        P[IDENT_ROWS] = np.array(V.IDENT_ROW, dtype=np.uint64)
        P.setflags(write=False)
        _cache[key] = P
    return _cache[key]


def encoding_rows(oracle, t):
    """((m, t, 32), row-level accept flags): term j of row i is pool[(i + j) mod m] (the pool's undecodable rows lie together, so
    most rows keep all their terms decodable), with E_i1 = encode(-D_i0) in the first decodable rows of NEG_ROWS's count and
    E_i1 = E_i0 in the next ones."""
    key = ("E", t)
    if key not in _cache:
        pool = S.encoding_pool(oracle)
        m = len(pool)
        E = np.stack([pool[(np.arange(m) + j) % m] for j in range(t)], axis=1).copy()
        if t >= 2:
            D, ok = oracle.ris_decompress(np.ascontiguousarray(E[:16, 0]))
            assert ok.all()
            E[NEG_ROWS, 1] = oracle.ris_compress(oracle.ed_neg(D[:8]))
            E[SAME_ROWS, 1] = E[SAME_ROWS, 0]
        E[IDENT_ROWS] = 0                                                     # the identity's encoding in every term
        ok =oracle.ris_decompress(np.ascontiguousarray(E.reshape(m * t, 32)))[1].reshape(m, t)
        rows_ok = ok.all(axis=1)
        assert (~rows_ok).sum() >= 4 and rows_ok.sum() >= 200, ((~rows_ok).sum(), rows_ok.sum())
        assert all((ok[:, j] == 0).any() for j in range(t))                   # an undecodable term in every position
        E.setflags(write=False)
        _cache[key] = (E, ok)
    return _cache[key]


def tile(K, n):
    return np.ascontiguousarray(np.tile(np.array(K, dtype=np.uint64).reshape(1, -1, 5), (n, 1, 1)))


def want_ed(oracle, t, K):
    key = ("want_ed", t, tuple(map(tuple, K)))
    if key not in _cache:
        P = point_rows(oracle, t)
        out = R.oracle_lincomb(oracle, P, tile(K, len(P)))
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def want_wire(oracle, t, K):
    key = ("want_wire", t, tuple(map(tuple, K)))
    if key not in _cache:
        E, _ = encoding_rows(oracle, t)
        out, ok = RR.oracle_ris_lincomb(oracle, E, tile(K, len(E)), None)
        out.setflags(write=False)
        ok.setflags(write=False)
        _cache[key] = (out, ok)
    return _cache[key]


def _planted_count():
    return IDENT_ROWS[-1] + 1


def want_ed_folded(oracle, t, K):
    """want_ed composed from the oracle's k_j * (pool row), computed once per scalar whatever the term position, folded with
    the oracle's Add in index order; the planted rows (which are no pool rows) straight from oracle_lincomb."""
    key = ("want_ed_folded", t, tuple(map(tuple, K)))
    if key not in _cache:
        pool, _ = S.point_pool(oracle)
        m, P = len(pool), point_rows(oracle, t)
        acc = None
        for j in range(t):
            q = np.ascontiguousarray(S.want_ed(oracle, pool, [int(x) for x in K[j]])[(np.arange(m) + 37 * j) % m])
            acc = q if acc is None else oracle.mt(oracle.ed_add, acc, q)
        acc = acc.copy()
        c = _planted_count()
        acc[:c] = R.oracle_lincomb(oracle, np.ascontiguousarray(P[:c]), tile(K, c))
        acc.setflags(write=False)
        _cache[key] = acc
    return _cache[key]


def want_ed_folded_bytes(oracle, t, K):
    """(bytes, ok) of the oracle's ed_compress of want_ed_folded."""
    key = ("want_ed_folded_bytes", t, tuple(map(tuple, K)))
    if key not in _cache:
        _cache[key] = oracle.mt(oracle.ed_compress, want_ed_folded(oracle, t, K))
    return _cache[key]


def want_wire_folded(oracle, t, K):
    """(bytes, ok) composed alike from the decoded pool."""
    key = ("want_wire_folded", t, tuple(map(tuple, K)))
    if key not in _cache:
        pool = S.encoding_pool(oracle)
        if "D" not in _cache:
            D, _ = oracle.ris_decompress(pool)
            D = np.ascontiguousarray(D)
            D.setflags(write=False)
            _cache["D"] = D
        D, m = _cache["D"], len(pool)
        E, ok_terms = encoding_rows(oracle, t)
        acc = None
        for j in range(t):
            q = np.ascontiguousarray(S.want_ed(oracle, D, [int(x) for x in K[j]])[(np.arange(m) + j) % m])
            acc = q if acc is None else oracle.mt(oracle.ed_add, acc, q)
        out = oracle.mt(oracle.ris_compress, acc).copy()
        ok = ok_terms.all(axis=1).astype(np.uint8)
        c = _planted_count()
        out[:c], ok[:c] = RR.oracle_ris_lincomb(oracle, np.ascontiguousarray(E[:c]), tile(K, c), None)
        out[ok == 0] = 0
        out.setflags(write=False)
        ok.setflags(write=False)
        _cache[key] = (out, ok)
    return _cache[key]


def planted_vectors(t, seed=SEED):
    """[(name, vector)]: the vectors the planted rows are for -- (k, k, 0, ..) (rows with P1 = -P0 sum to the identity), (k, k,
    random ..), (1, L - 1, ..), one zero among non-zero scalars (first and last position), all zero, all one."""
    rng = random.Random(seed + t)
    rnd = lambda: pm.limbs(rng.randrange(1 << 252))
    k = rnd()
    out = [("all zero", [[0] * 5] * t), ("all one", [pm.limbs(1)] * t)]
    if t >= 2:
        out += [("(k, k, 0..)", [k, k] + [[0] * 5] * (t - 2)), ("(k, k, random..)", [k, k] + [rnd() for _ in range(t - 2)]),
                ("(1, L - 1, random..)", [pm.limbs(1), pm.limbs(pm.L - 1)] + [rnd() for _ in range(t - 2)])]
        for j in (0, t - 1):
            out.append(("zero at %d" % j, [[0] * 5 if i == j else rnd() for i in range(t)]))
    return out


def edge_vectors(t, scalars, seed=SEED):
    """[(name, vector)]: the scalars of `scalars` t at a time, scalar e at term position e mod t, random 252-bit scalars where the
    list runs out."""
    rng = random.Random(seed + 100 + t)
    out = []
    for v in range(0, len(scalars), t):
        out.append(("scalars %d..%d" % (v, v + t - 1), [list(scalars[v + i]) if v + i < len(scalars) else pm.limbs(rng.randrange(1 << 252)) for i in range(t)]))
    return out


def each_position_vectors(t, scalars, seed=SEED):
    """[(name, vector)]: every scalar of `scalars` in each term position in turn; the other positions hold random scalars that
    depend on the position alone (eight in all, so that the oracle's products are shared between the vectors)."""
    fill = S.random_scalars(8, seed + 7)
    return [("scalar %d at %d" % (e, j), [list(s) if i == j else fill[i] for i in range(t)]) for e, s in enumerate(scalars) for j in range(t)]
