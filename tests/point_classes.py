"""Valid curve points by order, built from the oracle only (CPU tier and GPU tier share this catalogue).

The curve has cofactor 8: beside the prime-order subgroup <B> (order L) there are points of order 2, 4 and 8 and of order
2L, 4L and 8L.  torsion() builds E[8] from a decoded point, classes() the point classes a batched backend for untrusted data
receives, scalars_for_torsion() the scalars on which "right mod L" and "right as an integer" part: L * P is a non-trivial
point of E[8] for every P outside <B>, so a result that was reduced mod L shows on the rows L, 2L, 4L and 8L +- 1.

Every constructor asserts that its rows are what they claim to be (orders, L-multiples, validity)."""
import numpy as np

from oracle import pymodel as pm
from tests import vectors as V

M52 = (1 << 52) - 1
CLASS_NAMES = ("subgroup", "torsion", "order_2L", "order_4L", "order_8L", "decoded")     # `scaled` cycles through these
EVEN_SUBGROUP = ("subgroup",)                                                            # the classes zc_ris_is_valid accepts whole


def ident_rows(n=1):
    return np.tile(np.array(V.IDENT_ROW, dtype=np.uint64), (n, 1))


def scalar_rows(value, n):
    return np.tile(np.array(pm.limbs(value), dtype=np.uint64), (n, 1))


def is_identity(oracle, rows):
    rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, 20)
    return oracle.ed_eq(rows, ident_rows(len(rows))) == 1


def order_in_e8(oracle, row):
    """The order (1, 2, 4 or 8) of a point of E[8], by repeated ed_double and ed_eq against the identity; None outside E[8]."""
    cur = np.ascontiguousarray(row, dtype=np.uint64).reshape(1, 20)
    for o in (1, 2, 4, 8):
        if is_identity(oracle, cur)[0]:
            return o
        cur = oracle.ed_double(cur)
    return None


def times_L(oracle, rows):
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    return oracle.mt(oracle.ed_scalar_mul, rows, scalar_rows(pm.L, len(rows)))


def normalised(oracle, rows):
    """(x, y, 1, x y) in canonical limbs."""
    xy, ok = oracle.ed_to_affine(rows)
    assert ok.all()
    one = scalar_rows(1, len(rows))
    return np.concatenate([xy, one, oracle.fe_mul(np.ascontiguousarray(xy[:, :5]), np.ascontiguousarray(xy[:, 5:]))], axis=1)


_torsion = {}


def torsion(oracle):
    """The eight points of E[8] as (8, 20) limb rows with Z = 1: row j = j * T8, T8 = L * Q for Q the decoding of the first
    small integer y whose L-multiple has order exactly 8."""
    if "rows" in _torsion:
        return _torsion["rows"].copy()
    t8 = None
    for y in range(2, 64):
        q, ok = oracle.ed_decompress(np.frombuffer(int(y).to_bytes(32, "little"), dtype=np.uint8).reshape(1, 32))
        if not ok[0]:
            continue
        assert oracle.ed_is_valid(q)[0] == 1
        cand = times_L(oracle, q)
        if order_in_e8(oracle, cand) == 8:
            t8 = cand
            break
    assert t8 is not None, "no small y decodes to a point whose L-multiple has order 8"
    rows = [ident_rows()]
    for _ in range(7):
        rows.append(oracle.ed_add(rows[-1], t8))
    rows = normalised(oracle, np.concatenate(rows))
    assert np.array_equal(rows[0], ident_rows()[0])
    assert [order_in_e8(oracle, r) for r in rows] == [1, 8, 4, 8, 2, 8, 4, 8]
    assert oracle.ed_is_valid(rows).all()
    assert rows[4].tolist() == [0] * 5 + pm.limbs(pm.P - 1) + pm.limbs(1) + [0] * 5          # 4 T8 = (0, -1)
    assert oracle.ed_eq(times_L(oracle, rows), rows[(pm.L % 8) * np.arange(8) % 8]).all()    # L = 3 (mod 8) acts on E[8]
    four = oracle.ed_coset4(ident_rows()).reshape(4, 20)
    small = [r for r in four if not is_identity(oracle, r)[0]]
    assert len(small) == 3
    # The reference's FOUR_COSET_GROUP[0] is (1, 0), which is not on this curve (a = -1: -1 + 0 != 1), so ed_coset4(identity)
    # holds two curve points beside the identity, (-sqrt(-1), 0) and (0, -1), and one reference-defined row that is none.
    on_curve = [r for r in small if oracle.ed_is_valid(r.reshape(1, 20))[0] == 1]
    assert len(on_curve) == 2 and [r.tolist() for r in small if oracle.ed_is_valid(r.reshape(1, 20))[0] == 0] == [pm.limbs(1) + [0] * 5 + pm.limbs(1) + [0] * 5]
    for r in on_curve:                                                                       # they are among the rows
        assert sum(int(oracle.ed_eq(r.reshape(1, 20), t.reshape(1, 20))[0]) for t in rows) == 1
    assert len({bytes(oracle.ed_compress(r.reshape(1, 20))[0]) for r in rows}) == 8
    _torsion["rows"] = rows
    return rows.copy()


def torsion_index(oracle, rows):
    """j with row == j * T8 for rows of E[8] (every row must be in E[8])."""
    tors = torsion(oracle)
    rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, 20)
    idx = np.full(len(rows), -1)
    for j in range(8):
        idx[oracle.mt(oracle.ed_eq, rows, np.tile(tors[j], (len(rows), 1))) == 1] = j
    assert (idx >= 0).all(), "rows outside E[8]"
    return idx


def subgroup(oracle, n, seed):
    """r_i * B, the rows of V.base_multiples, on all host cores."""
    k = V.rand_scalars_np(n, seed, bits=249)
    b = np.tile(np.array(sum(pm.pt_limbs(pm.BASEPOINT), []), dtype=np.uint64), (n, 1))
    return oracle.mt(oracle.ed_scalar_mul, b, k)


def decoded(oracle, n, seed):
    """ed_decompress of seeded random bytes (y below 2^252, either sign): the first n that decode."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((0, 20), dtype=np.uint64)
    while len(rows) < n:
        b = rng.integers(0, 256, size=(2 * n + 16, 32), dtype=np.uint8)
        b[:, 31] &= 0x8F
        pts, ok = oracle.ed_decompress(b)
        rows = np.concatenate([rows, pts[ok == 1]])
    return np.ascontiguousarray(rows[:n])


def scale(oracle, rows, seed):
    """(lambda X, lambda Y, lambda Z, lambda T) for a seeded non-zero lambda per row: the same points in other coordinates."""
    lam = V.rand_fe_np(len(rows), seed)
    lam[:, 0] |= np.uint64(1)                                                                # odd, so not zero
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    return np.concatenate([oracle.fe_mul(np.ascontiguousarray(rows[:, 5 * c:5 * c + 5]), lam) for c in range(4)], axis=1)


def scaled_origin(n):
    """[(class name, row of that class)] for the rows of classes(..)['scaled']."""
    k = len(CLASS_NAMES)
    return [(CLASS_NAMES[i % k], (i // k) % n) for i in range(n)]


_classes = {}


def classes(oracle, n, seed):
    """name -> (n, 20): subgroup, torsion, order_2L / _4L / _8L, decoded, and scaled (scaled_origin(n) names its rows)."""
    key = (n, seed)
    if key in _classes:
        return {k: v.copy() for k, v in _classes[key].items()}
    tors = torsion(oracle)
    C = {"subgroup": subgroup(oracle, n, seed)}
    C["torsion"] = tors[np.arange(n) % 8]
    mixed = {"order_2L": [4], "order_4L": [2, 6], "order_8L": [1, 3, 5, 7]}
    for s, (name, js) in enumerate(mixed.items()):
        j = np.array(js)[np.arange(n) % len(js)]
        C[name] = oracle.mt(oracle.ed_add, subgroup(oracle, n, seed + 1 + s), tors[j])
        lp = times_L(oracle, C[name])
        assert oracle.ed_eq(lp, tors[(pm.L % 8) * j % 8]).all() and not is_identity(oracle, lp).any(), name
        assert {order_in_e8(oracle, r) for r in lp[:8]} == {int(name[6])}
    C["decoded"] = decoded(oracle, n, seed + 5)
    orders = {order_in_e8(oracle, r) for r in times_L(oracle, C["decoded"])}
    assert None not in orders and len(orders) >= 3, orders
    src = np.stack([C[name][i] for name, i in scaled_origin(n)])
    C["scaled"] = scale(oracle, src, seed + 6)
    if n >= 6 * 5:
        x0 = [r for r in C["scaled"] if not r[0:5].any()]                                    # (0, l, l, 0) and (0, -l, l, 0)
        assert any(np.array_equal(r[5:10], r[10:15]) for r in x0) and any(not np.array_equal(r[5:10], r[10:15]) for r in x0)
        assert all(r[10:15].tolist() != pm.limbs(1) for r in x0)
    assert oracle.mt(oracle.ed_eq, C["scaled"], src).all()
    for name, rows in C.items():
        assert rows.shape == (n, 20) and rows.dtype == np.uint64 and (rows <= M52).all(), name
        assert oracle.mt(oracle.ed_is_valid, rows).all(), name
    _classes[key] = C
    return {k: v.copy() for k, v in C.items()}


def in_even_subgroup(oracle, C):
    """name -> (n,) bool: the rows of C = classes(..) that lie in <B> (what zc_ris_is_valid accepts).  By construction: all of
    `subgroup`, the identity among `torsion`, none of the mixed orders; a decoded point is in <B> when its L-multiple is the
    identity (one in eight); a scaled row where its origin is."""
    n = len(C["subgroup"])
    out = {name: np.full(n, name in EVEN_SUBGROUP) for name in CLASS_NAMES}
    out["torsion"] = np.arange(n) % 8 == 0
    out["decoded"] = is_identity(oracle, times_L(oracle, C["decoded"]))
    out["scaled"] = np.array([bool(out[name][i]) for name, i in scaled_origin(n)])
    return out


def effective_scalar(k):
    """The integer the reference's double_and_add really multiplies by: it walks the bits of k from the bottom until the low
    256 bits of what is left are zero (its loop test compares 32-byte encodings), so raw limbs >= 2^256 may stop early."""
    k, eff, i = int(k), 0, 0
    while k % (1 << 256):
        eff |= (k & 1) << i
        k >>= 1
        i += 1
    return eff


def edge_scalars():
    """The named scalars of scalars_for_torsion(), as integers."""
    L = pm.L
    return [0, 1, 7, 8, 9, L - 1, L, L + 1, 2 * L, 4 * L, 8 * L - 1, 8 * L, 8 * L + 1, (1 << 252) - 1]


def scalars_for_torsion():
    """Raw limb rows: small scalars, the multiples of L around which E[8] shows, dense patterns and the raw edges >= 2^256."""
    rows = np.array([pm.limbs(v) for v in edge_scalars()] + [[M52] * 5], dtype=np.uint64)
    assert (rows <= M52).all()
    return np.concatenate([rows, V.raw_scalar_edges()])


def interleave(C, names=None):
    """Rows of the classes taken in turn (class 0 row 0, class 1 row 0, ...): every wave holds all of them.
    Returns (rows, class name per row)."""
    names = list(names or C.keys())
    n = len(C[names[0]])
    rows = np.stack([C[names[i % len(names)]][i // len(names)] for i in range(n * len(names))])
    return rows, [names[i % len(names)] for i in range(n * len(names))]
