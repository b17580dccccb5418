"""Inputs and the expected values shared by the zc_ris_lincomb tests (CPU emulation tier and GPU tier).

The expected bytes are always composed from the oracle's own functions:
want = ris_compress(((k0 D0 + k1 D1) + ...) + kB B) with D_j, ok_j = ris_decompress(bytes), the reference's Mul<Scalar> and
Add in index order, B = pymodel's BASEPOINT; 32 zero bytes and ok = 0 where any ok_j == 0.  Every row is compared, all 32
bytes and the mask."""
import numpy as np

from oracle import pymodel as pm
from tests import lincomb_rows as R
from tests import vectors as V

# (terms, base term) pairs of the row-family tests: with a base term the scalar slots stop at eight in all
CASES = [(1, True), (2, True), (4, True), (5, True), (7, True), (1, False), (3, False), (8, False)]
BAD_FAMILIES = ["random bytes", "s >= p", "p - s of a valid s", "top bit set", "undecodable under a zero scalar"]


def basepoint_rows(n):
    return np.tile(np.array(sum(pm.pt_limbs(pm.BASEPOINT), []), dtype=np.uint64), (n, 1))


def oracle_ris_lincomb(oracle, E, K, KB=None):
    """(want (n, 32) uint8, ok (n,) uint8) of E (n, t, 32), K (n, t, 5), KB (n, 5) or None."""
    E, K = np.ascontiguousarray(E, dtype=np.uint8), np.ascontiguousarray(K, dtype=np.uint64)
    n, t = E.shape[:2]
    D, okj = oracle.mt(oracle.ris_decompress, E.reshape(n * t, 32))
    ok = okj.reshape(n, t).all(axis=1)
    acc = R.oracle_lincomb(oracle, D.reshape(n, t, 20), K)
    if KB is not None:
        acc = oracle.mt(oracle.ed_add, acc, oracle.mt(oracle.ed_scalar_mul, basepoint_rows(n), np.ascontiguousarray(KB, dtype=np.uint64)))
    want = oracle.mt(oracle.ris_compress, acc).copy()
    want[~ok] = 0
    return want, ok.astype(np.uint8)


def le32(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint8)


def bad_encoding(family, valid, rng):
    """An encoding the reference refuses (random bytes: refuses about seven times in eight), from the 32 bytes of a valid one."""
    s = int.from_bytes(bytes(valid), "little")
    if family == 0:
        b = np.frombuffer(rng.bytes(32), dtype=np.uint8).copy()
        b[31] &= 0x0F
        return b
    if family == 1:
        return le32(pm.P + (s % 1000))                                # not canonical
    if family == 3:
        b = np.array(valid, dtype=np.uint8)
        b[31] |= 0x80
        return b
    return le32(pm.P - s)                                             # negative (p itself for s = 0: not canonical)


def base_scalars(n, seed):
    """(n, 5) base scalars: 252-bit random values with 0, 1, L, L - 1, all limbs 2^52 - 1 and the raw patterns at or above
    2^256 written over rows 2, 9, 16, ..."""
    KB = V.rand_scalars_np(n, seed, bits=252)
    edges = [[0] * 5, [1, 0, 0, 0, 0], pm.limbs(pm.L), pm.limbs(pm.L - 1), [(1 << 52) - 1] * 5] + [list(map(int, r)) for r in V.raw_scalar_edges()]
    for idx, pat in enumerate(edges):
        pos = 2 + 7 * idx
        if pos < n:
            KB[pos] = pat
    return KB


def ris_lincomb_rows(oracle, n, t, seed, base, points=None, compress=None):
    """(E (n, t, 32), K (n, t, 5), KB (n, 5) or None, planted): the encodings of lincomb_rows' points and its scalars (every
    planted scalar and point family, rows 3, 10, 17, ...), and every family of BAD_FAMILIES in every term position written
    over rows 5, 12, 19, ...; planted = the number of rows that hold one.  points(count, seed) / compress(points) supply the
    points and their encodings (default: the oracle's; large GPU batches take both from entry points that are not under test)."""
    P, K, _ = R.lincomb_rows(oracle, n, t, seed, points=points)
    compress = compress or (lambda pts: oracle.mt(oracle.ris_compress, pts))
    E = np.array(compress(P.reshape(n * t, 20)), dtype=np.uint8).reshape(n, t, 32)
    rng = np.random.default_rng(seed + 5)
    planted = 0
    for j in range(t):
        for family in range(len(BAD_FAMILIES)):
            pos = 5 + 7 * planted
            assert pos < n, "batch too small for the planted encodings"
            E[pos, j] = bad_encoding(family, E[pos, j], rng)
            if family == 4:
                K[pos, j] = 0
            planted += 1
    return E, K, (base_scalars(n, seed + 6) if base else None), planted


def assert_same_bytes(got, want):
    (gb, gok), (wb, wok) = got, want
    gb, gok = np.asarray(gb), np.asarray(gok)
    assert gb.shape == wb.shape and gb.dtype == np.uint8 and gok.shape == wok.shape
    rows = np.flatnonzero((gb != wb).any(axis=1) | (gok != wok))
    assert len(rows) == 0, "rows whose bytes or mask differ: %s" % rows[:16]
