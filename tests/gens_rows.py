"""Generator lists, scalar rows and expected results for the tests of the generator sets (zc_gens_create, zc_ed_mul_gens,
zc_ris_mul_gens_compress: CPU emulation, planted defects and GPU tier).

Generators come from the classes of tests/point_classes.py; the scalars of a row from one pool -- the radix-256 edge list of
tests/kill_vectors.py (recoding_scalars: runs of 0x80 / 0x7F / 0xFF bytes, values at bits 248..259, L - 1, L, 0), the raw patterns
at or above 2^256 of tests/vectors.py on both sides of the early-stop rule, limbs with bits from 2^52 up set, random 252-bit
values -- laid out so that every scalar of the pool stands in every term position once.  At most POOL rows per count, repeated
for longer batches.  The oracle's answers are its own Mul<Scalar>, Add and ris_compress in index order (tests/lincomb_rows.py),
computed once per count and cached."""
import ctypes as C

import numpy as np

from oracle import pymodel as pm
from tests import kill_vectors as KV
from tests import lincomb_rows as R
from tests import point_classes as PC
from tests import vectors as V

SEED = V.SEED + 0x6E45
COUNTS = (1, 2, 3, 8)
M52 = (1 << 52) - 1
GARBAGE_T = [0x123456789ABCD, 0xFEDCBA987654, 7, 0, 0xFFFFFFFFFFFFF]      # what T holds where the library must not read it

_cache = {}


def basepoint():
    return np.array([sum(pm.pt_limbs(pm.BASEPOINT), [])], dtype=np.uint64)


def generators(oracle, count):
    """(count, 20), read-only: 1: a mixed-order point with Z != 1; 2: G and -G (prime order); 3: a point of order 4L twice and a
    point of order 8; 8: prime order, the identity, order 4, order 2L, a prime-order point with Z != 1, a decoded point, order 8L
    and the basepoint.  T holds garbage wherever Z != 1 (the library reads X, Y and Z only)."""
    key = ("G", count)
    if key not in _cache:
        cl = PC.classes(oracle, 8, SEED)
        origin = PC.scaled_origin(8)
        mixed_scaled = cl["scaled"][origin.index(("order_8L", 0))]
        sub_scaled = cl["scaled"][origin.index(("subgroup", 0))]
        lists = {
            1: [mixed_scaled],
            2: [cl["subgroup"][0], oracle.ed_neg(cl["subgroup"][:1])[0]],
            3: [cl["order_4L"][0], cl["order_4L"][0], cl["torsion"][1]],
            8: [cl["subgroup"][1], PC.ident_rows(1)[0], cl["torsion"][2], cl["order_2L"][0], sub_scaled, cl["decoded"][0], cl["order_8L"][1], basepoint()[0]],
        }
        G = np.array(lists[count], dtype=np.uint64)
        assert G.shape == (count, 20) and oracle.ed_is_valid(G).all()
        not_one = [j for j in range(count) if G[j, 10:15].tolist() != pm.limbs(1)]
        assert not_one
        G[not_one, 15:] = np.array(GARBAGE_T, dtype=np.uint64)
        G.setflags(write=False)
        _cache[key] = G
    return _cache[key]


def with_true_t(oracle, G):
    """G with T = X Y / Z in every record: what the oracle multiplies."""
    G = np.array(G, dtype=np.uint64)
    xy, ok = oracle.ed_to_affine(G)
    assert ok.all()
    zt = oracle.fe_mul(np.ascontiguousarray(xy[:, :5]), np.ascontiguousarray(xy[:, 5:]))          # x y
    G[:, 15:] = oracle.fe_mul(zt, np.ascontiguousarray(G[:, 10:15]))                              # T = x y Z
    return G


def scalar_pool():
    """(POOL, 5) raw limb rows and the same with the bits from 2^52 up cleared (what the library multiplies by)."""
    if "pool" not in _cache:
        edges = [pm.limbs(v) for v in KV.recoding_scalars()]
        raw = [r for r in V.raw_scalar_edges(6).tolist() if r not in edges]
        rnd = V.rand_scalars_np(POOL - len(edges) - len(raw) - 4, SEED + 1, bits=252).tolist()
        dirty = [[w | (0xABC << 52) for w in edges[3]], [rnd[0][0] | (1 << 63)] + rnd[0][1:], [w | (1 << 52) for w in pm.limbs(pm.L - 1)],
                 [0, 0, 0, 0, (1 << 50) | (0xF << 52)]]
        pool = np.array(edges + raw + dirty + rnd, dtype=np.uint64)
        assert len(pool) == POOL and len({r.tobytes() for r in pool}) == POOL and (pool[:len(edges) + len(raw)] <= M52).all() and (pool[len(edges) + len(raw):][:4] > M52).any(axis=1).all()
        at_256 = pool[:, 4] & np.uint64(M52) >= np.uint64(1 << 48)
        assert at_256.sum() >= 30
        pool.setflags(write=False)
        _cache["pool"] = (pool, pool & np.uint64(M52))
    return _cache["pool"]


POOL = 96
TABLE_WORDS = 33 * 128 * 32                        # one generator's comb: 33 x 128 records of 128 bytes
STEP = 13                                           # term j of row i is pool[(i + 13 j) mod 96]: every scalar in every position


def scalars(count, n=POOL):
    """(n, count, 5) raw rows, row i = distinct row i mod POOL."""
    pool, _ = scalar_pool()
    i = np.arange(n) % POOL
    return np.ascontiguousarray(np.stack([pool[(i + STEP * j) % POOL] for j in range(count)], axis=1))


def want(oracle, count, n=POOL):
    """(points (n, 20), bytes (n, 32)): the oracle's ((k_0 G_0 + k_1 G_1) + ...) and its ris_compress."""
    key = ("want", count)
    if key not in _cache:
        _, clean = scalar_pool()
        i = np.arange(POOL)
        K = np.ascontiguousarray(np.stack([clean[(i + STEP * j) % POOL] for j in range(count)], axis=1))
        P = np.ascontiguousarray(np.tile(with_true_t(oracle, generators(oracle, count))[None], (POOL, 1, 1)))
        pts = R.oracle_lincomb(oracle, P, K)
        enc = oracle.mt(oracle.ris_compress, pts)
        pts.setflags(write=False)
        enc.setflags(write=False)
        _cache[key] = (pts, enc)
    pts, enc = _cache[key]
    i = np.arange(n) % POOL
    return pts[i], enc[i]


def want_base(oracle, n=POOL):
    """The same for the one-generator list [B]."""
    if "want_base" not in _cache:
        _, clean = scalar_pool()
        pts = oracle.mt(oracle.ed_scalar_mul, np.ascontiguousarray(np.tile(basepoint(), (POOL, 1))), np.ascontiguousarray(clean))
        _cache["want_base"] = (pts, oracle.mt(oracle.ris_compress, pts))
    pts, enc = _cache["want_base"]
    i = np.arange(n) % POOL
    return pts[i], enc[i]


def refused_lists(oracle):
    """[(name, (count, 20) points, index of the first generator that is no curve point)]: a point off the curve, Z = 0 (with
    X = 0, so that the projective equation holds), Z = the limbs of p, each behind valid generators and in front of another bad one."""
    good = generators(oracle, 8)
    off = good[0].copy()
    off[5] ^= np.uint64(1)                                                       # y changed in its lowest bit
    z0 = np.array([0] * 5 + pm.limbs(5) + [0] * 5 + [0] * 5, dtype=np.uint64)
    zp = good[3].copy()
    zp[10:15] = pm.limbs(pm.P)
    assert oracle.ed_is_valid(np.stack([off, z0])).tolist() == [0, 1]               # Z = 0 passes the projective equation
    return [("off the curve", np.stack([good[0], good[1], off, z0]), 2), ("Z = 0", np.stack([z0]), 0),
            ("Z = limbs of p", np.stack([good[2], zp, off]), 1), ("Z = 0 last", np.stack([good[k] for k in range(7)] + [z0]), 7)]


# ------------------------------------------------------------------ the host-emulation library (tests/emul/gens_emul.cpp)
def _p(a):
    return C.c_void_p(a.ctypes.data)


class Emul:
    """One build of tests/emul/gens_emul.cpp.  Tables are exact-size arrays between two guard words; outputs are framed."""

    def __init__(self, lib):
        self.lib = lib
        self.words = TABLE_WORDS

    def _tables(self, count):
        buf = np.full(count * self.words + 8, 0xA5A5A5A5, dtype=np.uint32)      # 16 bytes of guard on either side
        return buf, buf[4:-4]

    def build(self, points):
        """(first bad generator or -1, tables)."""
        points = np.ascontiguousarray(points, dtype=np.uint64)
        before = points.copy()
        buf, t = self._tables(len(points))
        bad = self.lib.emul_gens_build(_p(points), C.c_size_t(len(points)), _p(t))
        assert (buf[:4] == 0xA5A5A5A5).all() and (buf[-4:] == 0xA5A5A5A5).all() and np.array_equal(points, before)
        return bad, t

    def base_table(self):
        buf, t = self._tables(1)
        self.lib.emul_base_table(_p(t))
        assert (buf[:4] == 0xA5A5A5A5).all() and (buf[-4:] == 0xA5A5A5A5).all()
        return t

    def _rows(self, fn, head, K, width, dtype):
        K = np.ascontiguousarray(K, dtype=np.uint64)
        before, n = K.copy(), len(K)
        fill = 0xA5
        buf = np.full(width * (n + 2), fill, dtype=dtype)
        out = buf[width:width * (n + 1)]
        fn(*head, _p(K), _p(out), C.c_size_t(n))
        assert (buf[:width] == fill).all() and (buf[width * (n + 1):] == fill).all() and np.array_equal(K, before)
        return out.reshape(n, width).copy()

    def ed(self, tables, K):
        return self._rows(self.lib.emul_ed_mul_gens, (_p(tables), C.c_size_t(K.shape[1])), K, 20, np.uint64)

    def wire(self, tables, K):
        return self._rows(self.lib.emul_ris_mul_gens_compress, (_p(tables), C.c_size_t(K.shape[1])), K, 32, np.uint8)

    def ed_base(self, table, K):
        return self._rows(self.lib.emul_ed_mul_base, (_p(table),), K, 20, np.uint64)

    def wire_base(self, table, K):
        return self._rows(self.lib.emul_ris_mul_base_compress, (_p(table),), K, 32, np.uint8)


def failures(lib, oracle, n=POOL + 37):
    """The checks of the emulation tier on one build, as labels of those that failed: per count "build", "ed" (group equality and
    compressed bytes against the oracle) and "wire" (bytes); "refusals"; "basepoint" ([B] against the emulated basepoint calls)."""
    em, failed = Emul(lib), []
    for count in COUNTS:
        bad, t = em.build(generators(oracle, count))
        if bad != -1:
            failed.append("build [count=%d]" % count)
            continue
        K = scalars(count, n)
        pts, enc = want(oracle, count, n)
        got = em.ed(t, K)
        same = oracle.mt(oracle.ed_eq, got, np.ascontiguousarray(pts)).all() and (got <= M52).all()
        if not (same and np.array_equal(oracle.mt(oracle.ris_compress, got), enc) and
                np.array_equal(oracle.mt(oracle.ed_compress, got)[0], oracle.mt(oracle.ed_compress, np.ascontiguousarray(pts))[0])):
            failed.append("ed [count=%d]" % count)
        if not np.array_equal(em.wire(t, K), enc):
            failed.append("wire [count=%d]" % count)
    for name, pts, first in refused_lists(oracle):
        if em.build(pts)[0] != first:
            failed.append("refusals [%s]" % name)
    bad, t = em.build(basepoint())
    K = scalars(1, n)[:, 0]
    base = em.base_table()
    wp, wb = want_base(oracle, n)
    if bad != -1 or not oracle.mt(oracle.ed_eq, em.ed(t, K[:, None]), em.ed_base(base, K)).all() or not np.array_equal(em.wire(t, K[:, None]), em.wire_base(base, K)) \
            or not np.array_equal(em.wire(t, K[:, None]), wb) or not oracle.mt(oracle.ed_eq, em.ed(t, K[:, None]), np.ascontiguousarray(wp)).all():
        failed.append("basepoint")
    return failed
