"""Rows and expected values for the scalar operations for protocols (zc_sc_from_bytes_wide / _mod_order, zc_sc_muladd,
zc_sc_invert), shared by the CPU emulation tier and the GPU tier.  Nothing here is in the reference: every expected value is
a Python integer computed with oracle.pymodel's L, limbs and from_limbs, from the VALUE a row holds,
val(w) = sum (w_i mod 2^52) 2^(52 i)."""
import random

import numpy as np

from oracle import pymodel as pm

L = pm.L
M52 = (1 << 52) - 1
ALL_ONES = (1 << 64) - 1
HIGH = 1 << 52                                      # a bit the value ignores


def value(words):
    return sum((int(w) & M52) << (52 * i) for i, w in enumerate(words))


def rows(vals):
    """Five 52-bit limbs per value (< 2^260)."""
    assert all(0 <= v < 1 << 260 for v in vals)
    return np.array([pm.limbs(v) for v in vals], dtype=np.uint64)


def values(arr):
    return [value(r) for r in np.asarray(arr).reshape(-1, 5)]


def canon_rows(vals):
    return rows([v % L for v in vals])


def to_bytes(vals, width):
    return np.frombuffer(b"".join(int(v).to_bytes(width, "little") for v in vals), dtype=np.uint8).reshape(len(vals), width).copy()


# ------------------------------------------------------------------ reduction of 64 / 32 bytes
def wide_edges():
    e = [0, 1, L - 1, L, L + 1, 2**256 - 1, 2**256, 2**256 + L, 2**511, 2**512 - 1]
    e += [k * L for k in (2, 255, 2**256, 2**262)]
    assert all(v < 2**512 for v in e)
    return e


def narrow_edges():
    return [v for v in wide_edges() if v < 2**256]


def reduction_values(width, n_random, seed, bits=True):
    """The edge values that fit `width` bytes, every single-bit input, n_random seeded random rows."""
    rng = random.Random(seed)
    top = 8 * width
    vals = [v for v in wide_edges() if v < 1 << top]
    if bits:
        vals += [1 << j for j in range(top)]
    return vals + [rng.getrandbits(top) for _ in range(n_random)]


# ------------------------------------------------------------------ a b + c
def muladd_families(n_random, seed):
    """(a, b, c) as (n, 5) uint64 word arrays: canonical random values; all three operands 2^260 - 1; words with bits >= 2^52
    set (ignored); a = 0; c = L - 1 with a b = 1."""
    rng = random.Random(seed)
    A, B, C = [], [], []

    def add(a, b, c):
        A.append(a), B.append(b), C.append(c)
    for _ in range(n_random):
        add(pm.limbs(rng.randrange(L)), pm.limbs(rng.randrange(L)), pm.limbs(rng.randrange(L)))
    add(*[pm.limbs(2**260 - 1)] * 3)
    add([ALL_ONES] * 5, [ALL_ONES] * 5, [ALL_ONES] * 5)
    for _ in range(8):                                                            # honest values under high bits
        add(*[[x | (rng.getrandbits(12) << 52) for x in pm.limbs(rng.randrange(L))] for _ in range(3)])
    for _ in range(4):                                                            # one operand at or above 2^249, the others honest
        ops = [pm.limbs(rng.randrange(L)) for _ in range(3)]
        ops[rng.randrange(3)] = pm.limbs(rng.getrandbits(260) | 1 << 259)
        add(*ops)
    add(pm.limbs(L - 1), pm.limbs(L - 1), pm.limbs(L - 1))
    add(pm.limbs(2**249 - 1), pm.limbs(2**249 - 1), pm.limbs(2**249 - 1))        # the largest operands of the one-pass form
    for _ in range(4):
        add([0] * 5, pm.limbs(rng.randrange(L)), pm.limbs(rng.randrange(L)))     # a = 0
        add([HIGH] * 5, pm.limbs(rng.randrange(L)), pm.limbs(rng.randrange(L)))  # a = 0 by value
        a = rng.randrange(1, L)
        add(pm.limbs(a), pm.limbs(pow(a, -1, L)), pm.limbs(L - 1))                # a b + c = L: the result is 0
    return tuple(np.array(x, dtype=np.uint64) for x in (A, B, C))


def muladd_expected(a, b, c):
    return canon_rows([x * y + z for x, y, z in zip(values(a), values(b), values(c))])


# ------------------------------------------------------------------ inversion
def invert_edges():
    """Word rows: 1, 2, L - 1, L - 2, (L + 1) / 2, the non-canonical L + 1 (its inverse is 1) and 2^260 - 1."""
    return rows([1, 2, L - 1, L - 2, (L + 1) // 2, L + 1, 2**260 - 1])


def zero_patterns():
    """[(name, five words)], all 0 mod L by value."""
    pats = [("zeros", [0] * 5)] + [("%d L" % k, pm.limbs(k * L)) for k in (1, 2, 255, 2047)] + [("high bits only", [HIGH, 0, 0, 0, ALL_ONES & ~M52])]
    assert all(value(w) % L == 0 for _, w in pats) and 2047 * L < 1 << 260 <= 2048 * L
    return pats


def random_invert_rows(n, seed):
    """Mostly canonical non-zero values, one row in eight a raw 260-bit pattern, one in sixteen with high bits set."""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        w = pm.limbs(rng.randrange(1, L)) if i % 8 else pm.limbs(rng.getrandbits(260))
        if i % 16 == 5:
            w = [x | (rng.getrandbits(12) << 52) for x in w]
        out.append(w)
    return np.array(out, dtype=np.uint64)


def invert_expected(a):
    """(canonical limbs of val^-1 mod L or zeros, ok)."""
    out, ok = [], []
    for v in values(a):
        v %= L
        out.append(pow(v, -1, L) if v else 0)
        ok.append(1 if v else 0)
    return rows(out), np.array(ok, dtype=np.uint8)


def plant_among(arr, planted, seed):
    """Write the rows `planted` over seeded positions of `arr` (as many as fit, first and last row included); returns the
    positions."""
    n, k = len(arr), min(len(planted), len(arr))
    rng = random.Random(seed)
    pos = sorted(set([0, n - 1][:k]) | set(rng.sample(range(n), k)))[:k]
    for p, row in zip(pos, planted[:k]):
        arr[p] = row
    return pos
