"""Rows, scalars and expected results for the tests of zc_ed_scalar_mul_shared and zc_ris_mul_shared (CPU emulation and GPU
tier): small pools of distinct rows, repeated for longer batches, and the oracle's answers for a pool computed once per scalar."""
import numpy as np

from oracle import pymodel as pm
from tests import hostile_rows as H
from tests import point_classes as PC
from tests import vectors as V

SEED = V.SEED + 0x5A4ED
T48 = 1 << 48
# at or above 2^256: the first stops early (low256 = 7 < 2^ctz(8) = 8: multiplies by 7), the second does not (all 260 bits count)
STOPS_EARLY = [7, 0, 0, 0, 8 * T48]
RUNS_ON = [8, 0, 0, 0, 8 * T48]

_cache = {}


def words(v):
    return pm.limbs(v)


def edge_scalars():
    """[five words]: small values around the window, the order L and its neighbours, the longest patterns, raw patterns at or above
    2^256 on both sides of the early-stop rule."""
    L = pm.L
    ints = [0, 1, 2, 3, 15, 16, 17, 31, 32, 33, L - 1, L, L + 1, 2 * L + 5, 1 << 249, (1 << 252) - 1, (1 << 256) - 1]
    return [words(v) for v in ints] + [STOPS_EARLY, RUNS_ON, [1, 0, 0, 0, 1 << 50], pm.limbs(2**256 + 5), [(1 << 52) - 1] * 5]


def random_scalars(n, seed=SEED + 1):
    return [[int(x) for x in r] for r in V.rand_scalars_np(n, seed, bits=252)]


def gpu_scalars():
    """The GPU tier's ten: 0, 1, L - 1, L + 1, 2^252 - 1, one pattern on each side of the early-stop rule, three random."""
    L = pm.L
    return [words(v) for v in (0, 1, L - 1, L + 1, (1 << 252) - 1)] + [STOPS_EARLY, RUNS_ON] + random_scalars(3, SEED + 2)


def point_pool(oracle, seeded=200):
    """At most 331 distinct curve points: every class of tests/point_classes (identity, E[8], mixed order, order L, decoded,
    other coordinates) interleaved, the identity, and `seeded` random multiples of the basepoint."""
    key = ("pt", seeded)
    if key not in _cache:
        rows, names = PC.interleave(PC.classes(oracle, 16, SEED))
        rows = np.ascontiguousarray(np.concatenate([rows, PC.ident_rows(1), V.base_multiples(oracle, seeded, SEED + 3)]))
        assert len(rows) <= 331
        rows.setflags(write=False)
        _cache[key] = (rows, names + ["identity"] + ["subgroup"] * seeded)
    return _cache[key]


def encoding_pool(oracle, seeded=200):
    """At most 331 distinct 32-byte rows: encodings of elligator images and of [0..15] B (the identity's 32 zero bytes among
    them), of points outside the even subgroup (whatever ris_compress makes of them), and undecodable rows."""
    key = ("enc", seeded)
    if key not in _cache:
        rng = np.random.default_rng(SEED + 4)
        ell = oracle.ris_compress(oracle.ris_from_uniform_bytes(rng.integers(0, 256, size=(seeded, 64), dtype=np.uint8)))
        mult = [pm.IDENT]
        for _ in range(15):
            mult.append(pm.ed_add(mult[-1], pm.BASEPOINT))
        small = oracle.ris_compress(V.pts_np(mult))
        other = oracle.ris_compress(PC.interleave(PC.classes(oracle, 16, SEED))[0])
        bad = np.stack([b for _, b in H.undecodable(oracle.ris_decompress)] * 2)
        junk = rng.integers(0, 256, size=(8, 32), dtype=np.uint8)
        rows = np.ascontiguousarray(np.concatenate([ell[: seeded // 2], small, bad[:2], other[:64], junk, ell[seeded // 2:], bad[2:]]))
        assert len(rows) <= 331 and not rows[seeded // 2].any()
        ok = oracle.ris_decompress(rows)[1]
        assert (ok == 0).sum() >= 4 and (ok == 1).sum() >= seeded
        rows.setflags(write=False)
        _cache[key] = rows
    return _cache[key]


def tile(k, n):
    return np.tile(np.array(k, dtype=np.uint64), (n, 1))


def want_ed(oracle, rows, k):
    """The reference's Mul<Scalar> of every row of the pool by k (cached per pool and scalar)."""
    key = ("want_ed", rows.ctypes.data, len(rows), tuple(k))
    if key not in _cache:
        out = oracle.mt(oracle.ed_scalar_mul, rows, tile(k, len(rows)))
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def want_wire(oracle, enc, k):
    """(bytes, ok) of the reference's decompress, Mul<Scalar>, compress (cached per pool and scalar)."""
    key = ("want_wire", enc.ctypes.data, len(enc), tuple(k))
    if key not in _cache:
        out, ok = oracle.mt(oracle.ris_roundtrip_mul, enc, tile(k, len(enc)))
        out.setflags(write=False)
        ok.setflags(write=False)
        _cache[key] = (out, ok)
    return _cache[key]
