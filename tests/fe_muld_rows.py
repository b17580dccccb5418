"""Inputs and checks for fp_mul_d (zc_curve.hip.h), shared by the emulation test, its planted defects and the sanitizer run.

An input is the nine 29-bit register limbs the routine receives (R-class: limbs 0..7 below 2^29, value below 3p).  The routine
returns d x as a residue, in whichever domain x lives, so the checks are on Python integers:
    value(fp_mul_d(x))                  = d x          (mod p), limbs below 2^29 + 2^30, value below 13 p
    fe_store_canon(fp_mul_d(x))         = d x R^-1 mod p, canonical     (the store leaves the Montgomery domain)
    fe_store_canon(mont_mul(D_M, x))    = the same limbs
model() is the routine step by step on integers; it finds the inputs that drive its intermediate u and its carries highest."""
import ctypes as C
import random

import numpy as np

from oracle import pymodel as pm
from tests import point_classes as PC
from tests import vectors as V

P = pm.P
MD = 126297
R = 1 << 261
RINV = pow(R, -1, P)
M29 = (1 << 29) - 1
TOP_MAX = 3 << 20                                    # the routine's input contract for limb 8
SEED = V.SEED + 0xD17
N_RANDOM = 100000
assert (pm.D + 1) * MD % P == 1


def reg(v):
    """Nine register limbs of the integer v (limb 8 keeps what is left)."""
    out = [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]
    assert out[8] <= TOP_MAX, hex(v)
    return out


def value(l):
    return sum(int(x) << (29 * i) for i, x in enumerate(l))


def model(l):
    """(u, largest carry, y) of the routine on register limbs l, every step as the header states it."""
    k = [(-pow(P, -1, MD) << (29 * i)) % MD for i in range(9)]
    s = sum(int(x) * ki for x, ki in zip(l, k))
    q = ((s >> 18) * ((1 << 48) // MD)) >> 32
    u = s - 4 * q * MD
    assert 0 <= u < 1 << 20 and (s - u) % MD == 0 and (value(l) + u * P) % MD == 0
    n = [(P >> (29 * i)) & M29 for i in range(8)] + [P >> 232]
    carry, top, v = MD, 0, []
    for i in range(9):
        acc = int(l[i]) + carry + u * n[i]
        v.append((-acc * pow(MD, -1, 1 << 29)) & M29)
        acc += v[-1] * MD
        assert acc & M29 == 0
        carry = acc >> 29
        top = max(top, carry if i < 8 else 0)
    assert carry == MD
    y = value([x ^ M29 for x in v])
    assert y * MD == value(l) + u * P
    return u, top, y


def named_inputs(oracle):
    """[(name, nine limbs)]: the values, the R-class extremes, the residues mod m, the search results and the T coordinates."""
    rng = random.Random(SEED)
    out = [("zero", reg(0)), ("one", reg(1)), ("p - 1", reg(P - 1)), ("p", reg(P)), ("mont(1)", reg(R % P)), ("mont(-1)", reg((P - 1) * R % P)),
           ("3p - 1", reg(3 * P - 1)), ("limbs 0..7 all ones, largest top limb", [M29] * 8 + [TOP_MAX]), ("limbs 0..7 all ones, top limb 0", [M29] * 8 + [0]),
           ("only the top limb", [0] * 8 + [TOP_MAX])]
    for i in range(9):
        out.append(("limb %d alone" % i, [0] * i + [M29 if i < 8 else TOP_MAX] + [0] * (8 - i)))
    for j in range(24):
        kk = rng.randrange(3 * P // MD)
        out.append(("multiple of m", reg(kk * MD)))
        out.append(("m - 1 mod m", reg(kk * MD + MD - 1)))
    out += [("m", reg(MD)), ("m - 1", reg(MD - 1)), ("m + 1", reg(MD + 1))]
    # u and the carries: the sum S moves by MD_K[0] per unit of limb 0, so a window of limb 0 under the largest limbs 1..8 walks
    # the Barrett remainder through its whole range at the largest S; the carry follows u N[i] + v_i m, searched on random limbs
    best_u, best_c = (0, None), (0, None)
    for x0 in range(M29 - 6000, M29 + 1):
        l = [x0] + [M29] * 7 + [TOP_MAX]
        u, c, _ = model(l)
        best_u = max(best_u, (u, l))
    for _ in range(4000):
        l = [rng.randrange(M29 - 255, M29 + 1) for _ in range(8)] + [rng.randrange(TOP_MAX + 1)]
        u, c, _ = model(l)
        best_u, best_c = max(best_u, (u, l)), max(best_c, (c, l))
    assert best_u[0] > 6 * MD and best_u[0] < 8.1 * MD and best_c[0] < 1 << 21
    out += [("largest u found (%d)" % best_u[0], best_u[1]), ("largest carry found (%d)" % best_c[0], best_c[1])]
    tors = PC.torsion(oracle)
    rows = np.concatenate([PC.ident_rows(), tors, V.base_multiples(oracle, 16, SEED)])
    assert not tors[4][15:].any() and not tors[0][15:].any()                              # T = 0 on the identity and on (0, -1)
    for r in rows:
        t = pm.from_limbs([int(x) for x in r[15:20]])
        out += [("T as loaded, Montgomery form", reg(t * R % P)), ("T as loaded, plain", reg(t))]
    return out


_cache = {}


def inputs(oracle):
    """(names, (n, 9) uint32 limbs, (n, 5) expected canonical limbs, [d x mod p]) -- built once."""
    if "v" not in _cache:
        named = named_inputs(oracle)
        rng = np.random.default_rng(SEED)
        rnd = rng.integers(0, 1 << 29, size=(N_RANDOM, 9), dtype=np.uint64)
        rnd[:, 8] = rng.integers(0, TOP_MAX + 1, size=N_RANDOM, dtype=np.uint64)
        x = np.concatenate([np.array([l for _, l in named], dtype=np.uint64), rnd]).astype(np.uint32)
        names = [nm for nm, _ in named] + ["random"] * N_RANDOM
        res = [pm.D * value(l) % P for l in x]
        want = np.array([pm.limbs(r * RINV % P) for r in res], dtype=np.uint64)
        _cache["v"] = (names, x, want, res)
    return _cache["v"]


def run(lib, x):
    n = len(x)
    x = np.ascontiguousarray(x, dtype=np.uint32)
    raw = np.zeros((n, 9), dtype=np.uint32)
    got, ref = np.zeros((n, 5), dtype=np.uint64), np.zeros((n, 5), dtype=np.uint64)
    lib.emul_fe_muld(C.c_void_p(x.ctypes.data), C.c_void_p(raw.ctypes.data), C.c_void_p(got.ctypes.data), C.c_void_p(ref.ctypes.data), C.c_size_t(n))
    return raw, got, ref


def failures(lib, oracle):
    """Names of the inputs on which the library misses one of the checks of the module docstring."""
    names, x, want, res = inputs(oracle)
    raw, got, ref = run(lib, x)
    bad = (got != want).any(axis=1) | (ref != want).any(axis=1) | (raw >= (1 << 29) + (1 << 30)).any(axis=1) | (raw[:, 8] >= 1 << 24)
    out = {i for i in np.nonzero(bad)[0]}
    for i in list(range(len(names) - N_RANDOM)) + list(range(len(names) - N_RANDOM, len(names), 97)):   # the integer check: named rows, a stride of the rest
        v = value(raw[i])
        if v % P != res[i] or v >= 13 * P:
            out.add(i)
    return ["%s [%d]" % (names[i], i) for i in sorted(out)]
