"""Rows, shapes and expected values for the scalar vector ops (zc_sc_sum_rows, zc_sc_dot_rows, zc_sc_powers), shared by the CPU
emulation tier, the planted defects and the GPU tier.  Nothing here is in the reference: every expected value is a Python
integer computed from the VALUE a record holds, val(w) = sum (w_i mod 2^52) 2^(52 i), reduced mod L.

Families of operands
  random   249-bit random scalars
  edges    the operands of scalar_ext_rows.muladd_families and 0, 1, L - 1, L, multiples of L up to 2047 L, 2^249 - 1, 2^249,
           2^260 - 1 and words with only bits >= 2^52 set, in a seeded order
  worst    every operand 2^260 - 1 under all-ones words: the largest columns and the largest sums a row of its length can have
Bases of the powers: 0 (and 0 by value: L, high bits only), 1, L - 1, an element of order 4, random and raw 260-bit values.

Shapes: n in {1, 63, 64, 65, 257} crossed sparsely with the general lengths, both sides of every threshold of the plan
(dusk_zerocaf_amd/csrc/zc_scvec_plan.h, read from its text) at n in {1, 3}, and one row of 16 * 2^16 + 5 terms."""
import ctypes as C
import functools
import os
import random
import re

import numpy as np

from oracle import pymodel as pm
from tests import scalar_ext_rows as SR
from tests.emul_build import CSRC

L, M52, ALL_ONES, HIGH = SR.L, SR.M52, SR.ALL_ONES, SR.HIGH
SEED = 2300
TOPBIT = 249
WORST = (1 << 260) - 1
BIG_ROW = 16 * (1 << 16) + 5
GENERAL_TERMS = [0, 1, 2, 3, 7, 8, 31, 32, 33, 64, 65, 511, 512, 513]
GENERAL_N = [1, 63, 64, 65, 257]
FAMILIES = ("random", "edges", "worst")
EDGE_RECORDS_MAX = 40000                            # the edge family runs on the shapes up to this many records


@functools.lru_cache(maxsize=None)
def plan_constants():
    """name -> value for every `constexpr size_t SCV_... = <integer>;` of the plan header."""
    text = open(os.path.join(CSRC, "zc_scvec_plan.h")).read()
    return {k: int(v) for k, v in re.findall(r"^constexpr size_t (SCV_[A-Z0-9_]+) = (\d+);", text, flags=re.M)}


def rows_thresholds():
    """Where parts changes (4, 16, 64, 256: four records per lane), where the block form ends (and the fold's nineteenth limb
    begins), where the two-kernel form begins, and a count of workgroups per row that changes from odd to even."""
    c = plan_constants()
    s = c["SCV_NOHI_MAX"]
    return [s, 4 * s, 16 * s, 64 * s, c["SCV_BLOCK_TERMS_MAX"], c["SCV_P256_MAX"], 3 * c["SCV_TWO_ROW_TERMS"]]


def pow_thresholds():
    c = plan_constants()
    s = c["SCV_POW_STAGE"] // 256
    return [s, 4 * s, 16 * s, 64 * s, c["SCV_POW_G256_MAX"], c["SCV_POW_G4096_MAX"]]


def _shapes(thresholds):
    out = []
    for i, t in enumerate(GENERAL_TERMS):
        out.append((GENERAL_N[i % 5], t))
        out.append((GENERAL_N[(i + 2) % 5], t))
    for t in thresholds:
        out += [(n, t + d) for n in (1, 3) for d in (0, 1)]
    out.append((1, BIG_ROW))
    seen = []
    for s in out:
        if s not in seen:
            seen.append(s)
    return seen


def row_shapes():
    """(n, terms) of the sums and dot products.  The last threshold is a bpr that is odd at the tree's second level (3 workgroups
    of a row against 4)."""
    return _shapes(rows_thresholds())


def pow_shapes():
    return _shapes(pow_thresholds())


# ------------------------------------------------------------------ operands
@functools.lru_cache(maxsize=None)
def edge_pool():
    a, b, c = SR.muladd_families(8, SEED + 1)
    pool = [list(map(int, r)) for arr in (a, b, c) for r in arr]
    vals = [0, 1, L - 1, L, 2 * L, 255 * L, 2047 * L, 2**TOPBIT - 1, 2**TOPBIT, WORST]
    pool += [pm.limbs(v) for v in vals] + [w for _, w in SR.zero_patterns()]
    pool += [[x | (0xfff << 52) for x in pm.limbs(v)] for v in vals]
    return pool


def fill(n, terms, family, seed):
    """(n, terms, 5) words."""
    rng = random.Random(seed)
    if family == "worst":
        return np.full((n, terms, 5), ALL_ONES, dtype=np.uint64)
    if family == "random":
        raw = np.frombuffer(rng.getrandbits(n * terms * 5 * 64 + 8).to_bytes(n * terms * 40 + 1, "little")[:n * terms * 40], dtype=np.uint64).reshape(n, terms, 5).copy()
        raw &= np.uint64(M52)
        raw[..., 4] &= np.uint64((1 << (TOPBIT - 208)) - 1)
        return raw
    pool = edge_pool()
    return np.array([pool[rng.randrange(len(pool))] for _ in range(n * terms)], dtype=np.uint64).reshape(n, terms, 5)


def vals(arr):
    """The values of an array of records, as an object array of Python integers of the leading shape."""
    a = np.asarray(arr)
    v = np.zeros(a.shape[:-1], dtype=object)
    for i in range(5):
        v = v + ((a[..., i] & np.uint64(M52)).astype(object) << (52 * i))
    return v


def canon(values):
    """(len, 5) canonical limbs of the residues."""
    return np.array([pm.limbs(int(v) % L) for v in values], dtype=np.uint64).reshape(-1, 5)


def sum_expected(a):
    return canon(vals(a).sum(axis=1)) if a.shape[1] else np.zeros((a.shape[0], 5), dtype=np.uint64)


def dot_expected(a, b):
    if not a.shape[1]:
        return np.zeros((a.shape[0], 5), dtype=np.uint64)
    return canon((vals(a) * vals(b)).sum(axis=1))


def bases(n, seed):
    """(n, 5) words: the edge bases first, then random canonical and raw values."""
    rng = random.Random(seed)
    q = next(q for q in range(3, 1000) if (L - 1) % q == 0)
    small = next(h for h in (pow(g, (L - 1) // q, L) for g in range(2, 50)) if h != 1)      # an element of order q
    assert pow(small, q, L) == 1 and q < 1000
    edge = [[0] * 5, pm.limbs(1), pm.limbs(L - 1), pm.limbs(small), pm.limbs(L), [HIGH, 0, 0, 0, ALL_ONES & ~M52], pm.limbs(WORST), [ALL_ONES] * 5, pm.limbs(L + 1), pm.limbs(2)]
    out = []
    for i in range(n):
        if n < len(edge):                           # few rows: a random base first, then edges that change with the shape
            out.append(pm.limbs(rng.randrange(L)) if i == 0 else edge[(seed + i) % len(edge)])
        else:
            out.append(edge[i] if i < len(edge) else pm.limbs(rng.randrange(L)) if i % 4 else pm.limbs(rng.getrandbits(260)))
    if n >= len(edge):
        rng.shuffle(out)
    return np.array(out, dtype=np.uint64).reshape(n, 5)


def powers_expected(x, terms):
    out = np.zeros((len(x), terms, 5), dtype=np.uint64)
    for i, v in enumerate(vals(x)):
        v, p = int(v) % L, 1
        for j in range(terms):
            out[i, j] = pm.limbs(p)
            p = p * v % L
    return out


@functools.lru_cache(maxsize=None)
def case(op, family, n, terms):
    """The inputs and the expected output of one case, made once per process and never changed: sum -> (a, want),
    dot / dot_shared -> (a, b, want), powers -> (x, want)."""
    seed = SEED + 7 * n + 13 * terms + FAMILIES.index(family) if family in FAMILIES else SEED + n + terms
    if op == "powers":
        x = bases(n, seed)
        res = (x, powers_expected(x, terms))
    else:
        a = fill(n, terms, family, seed)
        if op == "sum":
            res = (a, canon([terms * WORST] * n) if family == "worst" else sum_expected(a))
        else:
            shared = op == "dot_shared"
            b = fill(1 if shared else n, terms, family, seed + 1)
            full = np.broadcast_to(b, a.shape)
            res = (a, b[0] if shared else b, canon([terms * WORST * WORST] * n) if family == "worst" else dot_expected(a, full))
    for r in res:
        r.setflags(write=False)
    return res


def cases(quick=False):
    """(op, family, n, terms) of the whole tier.  quick: without the shapes of more than 2^17 records (the GPU tier and the
    emulation run all of them; the planted defects do not need them)."""
    out = []
    for n, t in row_shapes():
        if quick and n * t > 1 << 17:
            continue
        for fam in FAMILIES:
            if fam == "edges" and n * t > EDGE_RECORDS_MAX:
                continue
            out += [("sum", fam, n, t), ("dot", fam, n, t)]
            if n > 1 or t in (8, 65, BIG_ROW):
                out.append(("dot_shared", fam, n, t))
    for n, t in pow_shapes():
        if quick and n * t > 1 << 17:
            continue
        out.append(("powers", "bases", n, t))
    return out


def label(op, family, n, terms):
    return "%s [%s n=%d terms=%d]" % (op, family, n, terms)


# ------------------------------------------------------------------ the emulation
GUARD = 3                                           # rows in front of and behind every output, which must stay as they were
FILL = 0xA5A5A5A5A5A5A5A5


class Emul:
    """One build of tests/emul/scvec_emul.cpp.  Outputs are framed: nothing outside rows 0 .. n-1 may be written."""

    def __init__(self, lib):
        self.lib = lib
        lib.emul_scvec_bound_failures.restype = C.c_ulonglong
        v, z = C.c_void_p, C.c_size_t
        lib.emul_sc_sum_rows.argtypes = [v, z, v, z]
        lib.emul_sc_dot_rows.argtypes = [v, v, z, C.c_uint, v, z]
        lib.emul_sc_powers.argtypes = [v, z, v, z]
        lib.emul_sc_slice_dot_const.argtypes = [v, v, z, v]
        lib.emul_sc_slice_sum_const.argtypes = [v, z, v]

    def constants(self):
        out = (C.c_ulonglong * 11)()
        self.lib.emul_scvec_constants(out)
        names = ("SCV_STAGE", "SCV_BLOCK_TERMS_MAX", "SCV_P256_MAX", "SCV_TWO_ROW_TERMS", "SCV_MAX_BPR", "SCV_CARRY_EVERY", "SCV_NOHI_MAX", "SCV_LONGEST_SLICE",
                 "SCV_POW_STAGE_STEPS", "SCV_POW_G256_MAX", "SCV_POW_G4096_MAX")
        return dict(zip(names, map(int, out)))

    def bound_failures(self):
        return int(self.lib.emul_scvec_bound_failures())

    @staticmethod
    def _framed(rows, width):
        buf = np.full((rows + 2 * GUARD, width), FILL, dtype=np.uint64)
        return buf, buf[GUARD:GUARD + rows]

    @staticmethod
    def _intact(buf, rows):
        assert (buf[:GUARD] == FILL).all() and (buf[GUARD + rows:] == FILL).all(), "written outside its rows"

    def run(self, op, *ins, terms=None):
        ins = [np.ascontiguousarray(x) for x in ins]
        p = lambda a: a.ctypes.data
        if op == "powers":
            x, = ins
            buf, out = self._framed(len(x) * terms, 5)
            self.lib.emul_sc_powers(p(x), terms, p(out), len(x))
            self._intact(buf, len(x) * terms)
            return out.reshape(len(x), terms, 5).copy()
        a = ins[0]
        n, t = a.shape[:2]
        buf, out = self._framed(n, 5)
        if op == "sum":
            self.lib.emul_sc_sum_rows(p(a), t, p(out), n)
        else:
            self.lib.emul_sc_dot_rows(p(a), p(ins[1]), t, 1 if op == "dot_shared" else 0, p(out), n)
        self._intact(buf, n)
        return out.copy()

    def slice_dot(self, a, b, m):
        a, b, out = np.array(a, dtype=np.uint64), np.array(b, dtype=np.uint64), np.zeros(5, dtype=np.uint64)
        self.lib.emul_sc_slice_dot_const(a.ctypes.data, b.ctypes.data, m, out.ctypes.data)
        return out

    def slice_sum(self, a, m):
        a, out = np.array(a, dtype=np.uint64), np.zeros(5, dtype=np.uint64)
        self.lib.emul_sc_slice_sum_const(a.ctypes.data, m, out.ctypes.data)
        return out


def slice_lengths():
    """Slice lengths around the carry passes and the nineteenth limb, and the longest slice a call can produce."""
    c = plan_constants()
    k, h = c["SCV_CARRY_EVERY"], c["SCV_NOHI_MAX"]
    longest = ((1 << 31) - 1 + 256 * c["SCV_MAX_BPR"] - 1) // (256 * c["SCV_MAX_BPR"])
    return sorted({1, h, h + 1, k - 1, k, k + 1, 2 * k, 2 * k + 1, 64, 65, 256, longest})


def failures(emul, quick=True):
    """Labels of the checks that fail on this build: every case against Python integers, the worst-magnitude slices, and
    (a -DZC_CHECK_BOUNDS build) the bounds."""
    bad = []
    for key in cases(quick):
        op, fam, n, t = key
        c = case(*key)
        got = emul.run(op, *c[:-1], terms=t)
        if not np.array_equal(got, c[-1]):
            bad.append(label(*key))
    worst = [ALL_ONES] * 5
    for m in slice_lengths():
        if emul.slice_dot(worst, worst, m).tolist() != pm.limbs(m * WORST * WORST % L):
            bad.append("slice_dot [worst m=%d]" % m)
        if emul.slice_sum(worst, m).tolist() != pm.limbs(m * WORST % L):
            bad.append("slice_sum [worst m=%d]" % m)
    if emul.bound_failures():
        bad.append("bounds")
    return bad
