"""Inputs and expected values shared by the zc_ris_lincomb_sum tests (CPU emulation tier and GPU tier; this module holds no
test).

The expected bytes are oracle.ris_compress(oracle.msm_naive_mt(points, w)) over the decodable rows: the points are the
oracle's ris_decompress of the encodings, the scalars the canonical w_ij = val(z_i) val(k_ij) mod L and, for the base term, the
pair (BASEPOINT, b = sum_i val(z_i) val(kB_i) mod L), all computed on Python integers from the VALUE a row's words hold,
val(w) = sum (w_i mod 2^52) 2^(52 i).  A row with an undecodable term contributes nothing."""
import random

import numpy as np

from oracle import pymodel as pm
from tests import ris_lincomb_rows as RR
from tests import scalar_ext_rows as SX
from tests import vectors as V

L = pm.L
ZERO32 = bytes(32)


def weights_and_terms(K, KB=None, Z=None):
    """(w (n, t) canonical ints, tb (n,) canonical ints or None) before the accept mask."""
    K = np.asarray(K, dtype=np.uint64)
    n, t = K.shape[:2]
    z = [1] * n if Z is None else [v % L for v in SX.values(Z)]
    kv = SX.values(K.reshape(n * t, 5))
    w = [[z[i] * kv[i * t + j] % L for j in range(t)] for i in range(n)]
    tb = None if KB is None else [z[i] * v % L for i, v in enumerate(SX.values(KB))]
    return w, tb


def decode_mask(oracle, E):
    """(points (n, t, 20) as the oracle decodes them, term flags (n, t) bool)."""
    E = np.ascontiguousarray(E, dtype=np.uint8)
    n, t = E.shape[:2]
    D, okj = oracle.mt(oracle.ris_decompress, E.reshape(n * t, 32))
    return D.reshape(n, t, 20), okj.reshape(n, t) != 0


def msm_pairs(oracle, E, K, KB=None, Z=None):
    """(points (m, 20), canonical scalars (m,) ints, ok (n,) uint8): the pairs of the accepted rows, the base term last."""
    D, flags = decode_mask(oracle, E)
    ok = flags.all(axis=1)
    w, tb = weights_and_terms(K, KB, Z)
    rows = np.flatnonzero(ok)
    P = D[rows].reshape(-1, 20)
    s = [x for i in rows for x in w[i]]
    if KB is not None:
        P = np.concatenate([P, RR.basepoint_rows(1)])
        s.append(sum(tb[i] for i in rows) % L)
    return np.ascontiguousarray(P), s, ok.astype(np.uint8)


def expected(oracle, E, K, KB=None, Z=None):
    """(the 32 bytes, ok (n,) uint8)."""
    P, s, ok = msm_pairs(oracle, E, K, KB, Z)
    if len(P) == 0:
        return ZERO32, ok
    return bytes(oracle.ris_compress(oracle.msm_naive_mt(P, SX.rows(s)))[0]), ok


def expected_pymodel(E, K, KB=None, Z=None):
    """The same on oracle/pymodel.py alone (small batches)."""
    E = np.asarray(E, dtype=np.uint8)
    n, t = E.shape[:2]
    w, tb = weights_and_terms(K, KB, Z)
    acc, b, ok = pm.IDENT, 0, []
    for i in range(n):
        pts = [pm.ris_decompress(bytes(E[i, j])) for j in range(t)]
        ok.append(int(all(p is not None for p in pts)))
        if not ok[-1]:
            continue
        for p, x in zip(pts, w[i]):
            acc = pm.ed_add(acc, pm.ed_scalar_mul(p, x))
        b += tb[i] if tb is not None else 0
    if tb is not None:
        acc = pm.ed_add(acc, pm.ed_scalar_mul(pm.BASEPOINT, b % L))
    return pm.ris_compress(acc), np.array(ok, dtype=np.uint8)


def scalar_patterns(seed):
    """Five-word rows: canonical, zero, L - 1, 128-bit, 1, and raw patterns at or above L (L itself, 2L, all limbs 2^52 - 1, words
    with bits at or above 2^52, the raw patterns at or above 2^256 of tests/vectors.py)."""
    rng = random.Random(seed)
    rows = [pm.limbs(rng.randrange(L)) for _ in range(4)] + [[0] * 5, pm.limbs(L - 1), pm.limbs(rng.getrandbits(128)), [1, 0, 0, 0, 0],
                                                             pm.limbs(L), pm.limbs(2 * L), [SX.M52] * 5, [SX.ALL_ONES] * 5,
                                                             [x | (rng.getrandbits(12) << 52) for x in pm.limbs(rng.randrange(L))]]
    rows += [w for _, w in SX.zero_patterns()[1:]]
    return np.concatenate([np.array(rows, dtype=np.uint64), V.raw_scalar_edges(8, seed)])


def mixed_scalars(count, seed):
    """(count, 5): 252-bit random rows (most of them at or above L) with scalar_patterns written over every third row, in turn."""
    out = V.rand_scalars_np(count, seed, bits=252)
    pats = scalar_patterns(seed + 1)
    for idx, pos in enumerate(range(1, count, 3)):
        out[pos] = pats[idx % len(pats)]
    return out


def canonical_scalars(count, seed):
    rng = random.Random(seed)
    return SX.rows([rng.randrange(L) for _ in range(count)])


def weights128(n, seed):
    rng = random.Random(seed)
    return SX.rows([rng.getrandbits(128) for _ in range(n)])


def encodings_of_multiples(oracle, count, seed, compress=None, points=None):
    """(count, 32) encodings of k B for seeded k, with the identity's 32 zero bytes and the sixteen [0..15] B among them (as many
    as fit) and one public key repeated over a stretch."""
    pts = points(count, seed) if points else V.base_multiples(oracle, count, seed)
    E = np.array((compress or (lambda p: oracle.mt(oracle.ris_compress, p)))(pts), dtype=np.uint8)
    small = [pm.IDENT]
    for _ in range(15):
        small.append(pm.ed_add(small[-1], pm.BASEPOINT))
    small = oracle.ris_compress(V.pts_np(small))
    assert not small[0].any()
    for idx, pos in enumerate(range(2, count, 5)):
        if idx >= 16:
            break
        E[pos] = small[idx]
    if count >= 64:
        E[count // 2:count // 2 + count // 8] = E[0]                  # the same public key in many rows
    return E


def bad_encodings(oracle, valid, seed):
    """One undecodable encoding per family of tests/ris_lincomb_rows.py (the zero-scalar family is the caller's), checked."""
    rng = np.random.default_rng(seed)
    out = []
    for family in range(4):
        while True:
            b = RR.bad_encoding(family, valid, rng)
            if not oracle.ris_decompress(b.reshape(1, 32))[1][0]:
                break
        out.append(b)
    return out


def plant_rejected(oracle, E, seed, every=17):
    """Undecodable encodings written over a term of every `every`-th row of E (n, t, 32) -- the first term and the last in
    turn, all families in turn -- and over the first and the last row when there are at least three; returns the rows."""
    n, t = E.shape[:2]
    rows = sorted(set(range(every - 1, n, every)) | ({0, n - 1} if n >= 3 else set()))
    for idx, i in enumerate(rows):
        j = 0 if idx % 2 == 0 else t - 1
        bad = bad_encodings(oracle, E[i, j], seed + idx)
        E[i, j] = bad[idx % len(bad)]
    return rows
