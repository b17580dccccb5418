"""GPU tier: torsion and mixed-order points (tests/point_classes.py) through every group-law path.

The inputs are valid curve points outside the prime-order subgroup -- E[8], orders 2L / 4L / 8L, decoded random bytes, and all
of them in scaled coordinates -- next to the everyday collisions (P beside -P, one point many times, the identity as
(0, l, l, 0)).  Every expectation is the CPU oracle's on the same arrays:
  (a) the reference's own formula sequences (add / sub / double / neg / coset4 / mul_by_pow_2, the ProjectivePoint rows, strict
      Mul<Scalar> at every launch shape and both left-to-right variants): every limb;
  (b) the windowed core, zc_ed_lincomb and the three MSMs: the same group element (ed_eq) with the same ed_compress bytes and
      ok flags -- never Ristretto bytes, which mean something on the even subgroup only -- and the closed form where the
      family has one (P - P = O, sums inside E[8] by index arithmetic mod 8);
  (c) predicates and codecs byte for byte.
A scalar that was reduced mod L, or replaced by L - k with a negated point, passes every basepoint-multiple test and fails
here: L * P is a non-trivial point of E[8] for the mixed orders."""
import numpy as np
import pytest

from oracle import pymodel as pm
from tests import lincomb_rows as LR
from tests import point_classes as PC
from tests import vectors as V

pytestmark = pytest.mark.gpu

STRICT, LTR_BIN, BINARY_NAF, FAST = 0, 1, 2, 16
SEED = V.SEED + 0x7C00
CAT_N = 64


@pytest.fixture(scope="module")
def eng():
    import dusk_zerocaf_amd as z
    e = z.Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def crossover(eng):
    """The smallest n zc_msm_batch takes the bucket regime for (at batch 2; the regime depends on n only)."""
    regimes = [eng.msm_batch_plan(n, 2)["regime"] for n in range(1, (1 << 14) + 1)]
    assert regimes[-1] == "buckets" and regimes[0] == "scalar_mul"
    x = regimes.index("buckets") + 1
    assert all(r == "buckets" for r in regimes[x - 1:]) and all(r == "scalar_mul" for r in regimes[:x - 1])
    return x


# ------------------------------------------------------------------ plumbing
def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.dtype == np.uint8 else a.view(np.int64)).cuda()


def to_host(t):
    if isinstance(t, np.ndarray):
        return t
    a = t.cpu().numpy()
    return a if a.dtype == np.uint8 else a.view(np.uint64)


def outs(r):
    return tuple(to_host(x) for x in (r if isinstance(r, tuple) else (r,)))


_cache = {}


def cached(key, make):
    """Inputs and oracle answers: computed once, shared between cases, never written to (callers copy)."""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def catalogue(oracle):
    return cached("catalogue", lambda: PC.classes(oracle, CAT_N, SEED))


def mixed_rows(oracle):
    """(rows, class name per row): the classes of the catalogue taken in turn, so that a wave holds all of them."""
    return cached("mixed", lambda: PC.interleave(catalogue(oracle)))


def tile(rows, n, shift=0):
    return np.ascontiguousarray(rows[(np.arange(n) + shift) % len(rows)])


def assert_rows_equal(got, want, what):
    got, want = outs(got), outs(want)
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape)
        bad = np.flatnonzero((g.reshape(len(g), -1) != w.reshape(len(w), -1)).any(axis=1))
        assert len(bad) == 0, "%s: output %d differs from the oracle on rows %s" % (what, k, bad[:16])


def assert_same_elements(oracle, got, want, what=""):
    """The same group elements: ed_eq = 1 and identical ed_compress bytes and ok flags, on every row."""
    got, want = np.ascontiguousarray(to_host(got), dtype=np.uint64).reshape(-1, 20), np.ascontiguousarray(want, dtype=np.uint64).reshape(-1, 20)
    assert got.shape == want.shape, what
    eq = oracle.mt(oracle.ed_eq, got, want)
    assert (eq == 1).all(), "%s: rows that differ as group elements: %s" % (what, np.flatnonzero(eq != 1)[:16])
    gb, gok = oracle.mt(oracle.ed_compress, got)
    wb, wok = oracle.mt(oracle.ed_compress, want)
    assert np.array_equal(gb, wb) and np.array_equal(gok, wok) and wok.all(), what


# ------------------------------------------------------------------ (a) the reference's formula sequences, every limb
def pair_rows(oracle):
    """(A, B, kinds): 300 pairs -- all 64 (T, T') of E[8] in plain and in scaled coordinates, then (P, P), (P, -P), (P, P + T)
    for every T in turn and (P, P in other coordinates) over the interleaved classes."""
    def make():
        T = PC.torsion(oracle)
        X, _ = mixed_rows(oracle)
        i, j = np.divmod(np.arange(64), 8)
        A, B, kinds = [T[i]], [T[j]], ["T, T'"] * 64
        A.append(PC.scale(oracle, T[i], SEED + 11))
        B.append(PC.scale(oracle, T[j], SEED + 12))
        kinds += ["scaled T, T'"] * 64
        P = X[:172]
        r = np.arange(172)
        other = {0: P, 1: oracle.ed_neg(P), 2: oracle.ed_add(P, T[(r // 4) % 8]), 3: PC.scale(oracle, P, SEED + 13)}
        A.append(P)
        B.append(np.stack([other[k % 4][k] for k in r]))
        kinds += [("P, P", "P, -P", "P, P + T", "P, scaled P")[k % 4] for k in r]
        A, B = np.concatenate(A), np.concatenate(B)
        assert A.shape == B.shape == (300, 20) and oracle.ed_is_valid(A).all() and oracle.ed_is_valid(B).all()
        s = oracle.ed_add(A, B)
        k = np.array(kinds)
        assert np.array_equal(PC.torsion_index(oracle, s[:64]), (i + j) % 8)                   # the closed forms of the pairs
        assert PC.is_identity(oracle, s[k == "P, -P"]).all() and oracle.ed_eq(s[k == "P, P"], oracle.ed_double(A[k == "P, P"])).all()
        assert oracle.ed_eq(A[k == "P, scaled P"], B[k == "P, scaled P"]).all() and not np.array_equal(A[k == "P, scaled P"], B[k == "P, scaled P"])
        return A, B, kinds
    return cached("pairs", make)


PAIR_OPS = [  # (entry point, oracle function, operands, extra argument)
    ("ed_add", "ed_add", "AB", ()), ("ed_add", "ed_add", "BA", ()), ("ed_sub", "ed_sub", "AB", ()), ("ed_double", "ed_double", "A", ()),
    ("ed_double", "ed_double", "B", ()), ("ed_neg", "ed_neg", "B", ()), ("ed_coset4", "ed_coset4", "B", ()),
    ("ed_mul_by_pow_2", "ed_mul_by_pow_2", "B", (3,)), ("ed_mul_by_cofactor", "ed_mul_by_pow_2", "B", None),
]


@pytest.mark.parametrize("n", [300, 4096 + 300])
def test_point_ops_every_limb(eng, oracle, n):
    """zc_ed_add / sub / double / neg / coset4 / mul_by_pow_2(3) / mul_by_cofactor at one lane per row (300) and on staged
    records (4096 + 300), host and device pointers."""
    A, B, _ = pair_rows(oracle)
    I = {"A": tile(A, n), "B": tile(B, n)}
    for name, ref, ops, extra in PAIR_OPS:
        args = [I[c] for c in ops]
        small = [I[c][:300] for c in ops]
        want = cached(("pair op", name, ops), lambda: oracle.mt(getattr(oracle, ref), *small, extra=(3,) if extra is None else extra))
        want = tile(want, n)
        for form, conv in (("host", lambda a: a), ("device", to_dev)):
            got = getattr(eng, name)(*[conv(a) for a in args], *(extra or ()))
            assert_rows_equal(got, want, (name, ops, n, form))


def test_projective_rows_every_limb(eng, oracle):
    """zc_proj_add / double / sub / scalar_mul / to_extended on the (X, Y, Z) images of the same pairs."""
    A, B, _ = pair_rows(oracle)
    A3, B3 = np.ascontiguousarray(A[:, :15]), np.ascontiguousarray(B[:, :15])
    K = tile(PC.scalars_for_torsion(), 300)
    for form, conv in (("host", lambda a: a), ("device", to_dev)):
        assert_rows_equal(eng.proj_add(conv(A3), conv(B3)), oracle.proj_add(A3, B3), ("proj_add", form))
        assert_rows_equal(eng.proj_sub(conv(A3), conv(B3)), oracle.proj_sub(A3, B3), ("proj_sub", form))
        assert_rows_equal(eng.proj_double(conv(B3)), oracle.proj_double(B3), ("proj_double", form))
        assert_rows_equal(eng.proj_to_extended(conv(B3)), oracle.proj_to_extended(B3), ("proj_to_extended", form))
        want = cached("proj mul", lambda: oracle.mt(oracle.proj_scalar_mul, B3, K))
        assert_rows_equal(eng.proj_scalar_mul(conv(B3), conv(K)), want, ("proj_scalar_mul", form))


def strict_inputs(oracle, n, canonical=False):
    """(P, K, planted): every class x every scalar of scalars_for_torsion() at rows 0 .. and, for the sizes that are compared
    on slices, again from row n // 2 on; the rest are the interleaved classes under random 252-bit scalars.
    canonical: scalars below L only (the left-to-right variants' contract).  planted = [(row, class, scalar index)]."""
    def make():
        C = catalogue(oracle)
        E = PC.scalars_for_torsion()
        if canonical:
            E = np.array([pm.limbs(v) for v in (0, 1, 7, 8, 9, pm.L - 1, pm.L - 2, (pm.L - 1) // 2, 1 << 248, (1 << 249) - 1)], dtype=np.uint64)
        X, _ = mixed_rows(oracle)
        P = tile(X, n, shift=3)
        K = V.rand_scalars_np(n, SEED + 20 + n, bits=249 if canonical else 252)
        planted = []
        for start in ([0] if n <= (1 << 14) + 1 else [0, n // 2]):
            pos = start
            for a, name in enumerate(C):
                for s in range(len(E)):
                    P[pos], K[pos] = C[name][(5 * s + a) % CAT_N], E[s]
                    planted.append((pos, name, s))
                    pos += 1
        assert pos <= n and len(planted) >= len(C) * len(E)
        return P, K, planted
    return cached(("strict inputs", n, canonical), make)


def compared_rows(n):
    return np.arange(n) if n <= (1 << 14) + 1 else np.r_[0:600, n // 2:n // 2 + 600, n - 300:n]


def strict_want(oracle, n):
    """(rows compared, the oracle's double_and_add on them); asserts that they hold every (class, edge scalar) combination."""
    def make():
        P, K, planted = strict_inputs(oracle, n)
        sel = compared_rows(n)
        inside = set(sel.tolist())
        combos = {(name, s) for pos, name, s in planted if pos in inside}
        assert combos == {(name, s) for name in catalogue(oracle) for s in range(len(PC.scalars_for_torsion()))}
        return sel, oracle.mt(oracle.ed_scalar_mul, P[sel], K[sel])
    return cached(("strict want", n), make)


@pytest.mark.parametrize("n", [1000, (1 << 14) + 1, (1 << 16) + 1])
def test_scalar_mul_strict_every_limb(eng, oracle, n):
    """Four lanes per element, the independent-chain kernel and one workgroup per 256 elements."""
    P, K, _ = strict_inputs(oracle, n)
    sel, want = strict_want(oracle, n)
    assert_rows_equal(eng.ed_scalar_mul(P, K)[sel], want, ("strict", n, "host"))
    assert_rows_equal(to_host(eng.ed_scalar_mul(to_dev(P), to_dev(K)))[sel], want, ("strict", n, "device"))


def scalar_cost(K):
    """numpy model of the cost the persistent kernel sorts by: bit length - 1 + popcount of the five 52-bit words."""
    K = K & np.uint64(PC.M52)
    pop = np.unpackbits(np.ascontiguousarray(K).view(np.uint8).reshape(len(K), -1), axis=1).sum(axis=1).astype(np.int64)
    bits = np.zeros(len(K), dtype=np.int64)
    for j in range(5):
        blen = np.frexp(K[:, j].astype(np.float64))[1]                                          # exact: the words are below 2^53
        bits = np.where(K[:, j] != 0, 52 * j + blen, bits)
    return np.where(bits > 0, bits - 1 + pop, 0)


def torsion_tile_inputs(oracle, n):
    """A second input set for the persistent kernel: two blocks of 192 rows of E[8] (plain and scaled), each block under one
    scalar whose cost no other row has.  Tiles are 64 consecutive rows of the cost-sorted order (dearest first), so whatever
    the order inside a cost class, each block fills at least two whole tiles: every lane of such a tile passes the gate of
    the doubling steps with a torsion point."""
    def make():
        X, _ = mixed_rows(oracle)
        T = PC.torsion(oracle)
        P = tile(X, n, shift=11)
        K = V.rand_scalars_np(n, SEED + 31, bits=252)
        both = np.concatenate([T, PC.scale(oracle, T, SEED + 32), PC.scale(oracle, T, SEED + 33)])
        blocks = []
        for start, k in ((1000, (1 << 252) - 1 - (1 << 100)), (n - 5000, sum(PC.M52 << (52 * i) for i in range(5)))):
            rows = np.arange(start, start + 192)
            P[rows], K[rows] = tile(both, 192, shift=start), pm.limbs(k)
            blocks.append(rows)
        cost = scalar_cost(K)
        for rows in blocks:
            c = cost[rows[0]]
            assert (cost[rows] == c).all() and (cost == c).sum() == len(rows)                  # the cost class is the block
            first = int((cost > c).sum())                                                       # its place in the sorted order
            tiles = [t for t in range(-(-first // 64), (first + len(rows)) // 64) if first <= 64 * t and 64 * t + 64 <= first + len(rows)]
            assert len(tiles) >= 2, "no tile of 64 torsion rows"
            PC.torsion_index(oracle, P[rows])                                                   # every row of the block is in E[8]
        sel = np.r_[0:300, blocks[0], blocks[1], n - 300:n]
        return P, K, sel, oracle.mt(oracle.ed_scalar_mul, P[sel], K[sel])
    return cached(("torsion tiles", n), make)


@pytest.mark.parametrize("sched", [None, "unified"], ids=["default schedule", "ZC_SCHED=unified"])
def test_scalar_mul_persistent_kernel_every_limb(eng, oracle, sched):
    """2^17 + 77: persistent waves over the cost-sorted permutation, doubling / generic steps and generic steps only."""
    n = (1 << 17) + 77
    P, K, _ = strict_inputs(oracle, n)
    sel, want = strict_want(oracle, n)
    P2, K2, sel2, want2 = torsion_tile_inputs(oracle, n)
    with V.tuned(ZC_SCHED=sched) as te:
        assert_rows_equal(te.ed_scalar_mul(P, K)[sel], want, ("strict", n, sched, "host"))
        assert_rows_equal(to_host(te.ed_scalar_mul(to_dev(P), to_dev(K)))[sel], want, ("strict", n, sched, "device"))
        assert_rows_equal(te.ed_scalar_mul(P2, K2)[sel2], want2, ("strict, tiles of torsion points", n, sched))


@pytest.mark.parametrize("mode", [LTR_BIN, BINARY_NAF], ids=["LTR_BIN", "BINARY_NAF"])
def test_scalar_mul_left_to_right_every_limb(eng, oracle, mode):
    n = 1500
    P, K, planted = strict_inputs(oracle, n, canonical=True)
    assert all(pm.from_limbs(k) < pm.L for k in K[:len(planted)]) and {name for _, name, _ in planted} == set(catalogue(oracle))
    want = cached(("ltr", mode), lambda: oracle.mt(oracle.ed_scalar_mul_mode, P, K, extra=(mode,)))
    assert_rows_equal(eng.ed_scalar_mul(P, K, flags=mode), want, ("mode", mode))


# ------------------------------------------------------------------ (b) the same group element
def test_scalar_mul_fast_same_elements(eng, oracle):
    """The windowed core: signed windows must represent the integer double_and_add walks, not its residue mod L."""
    n = 2048 + 5
    P, K, planted = strict_inputs(oracle, n)
    assert len(planted) == len(catalogue(oracle)) * len(PC.scalars_for_torsion())
    want = cached("fast want", lambda: oracle.mt(oracle.ed_scalar_mul, P, K))
    # the rows that tell an integer from a residue: L * (a point outside the subgroup) is a non-trivial point of E[8]
    rows = [pos for pos, name, s in planted if name == "order_8L" and pm.from_limbs(PC.scalars_for_torsion()[s]) == pm.L]
    assert rows and not PC.is_identity(oracle, want[rows]).any()
    assert_same_elements(oracle, eng.ed_scalar_mul(P, K, flags=FAST), want, "fast, host")
    assert_same_elements(oracle, eng.ed_scalar_mul(to_dev(P), to_dev(K), flags=FAST), want, "fast, device")


def lincomb_inputs(oracle, t):
    def make():
        n = 257
        C = catalogue(oracle)
        X, _ = mixed_rows(oracle)
        T = PC.torsion(oracle)
        E = PC.scalars_for_torsion()
        P = tile(X, n * t, shift=t).reshape(n, t, 20).copy()
        K = V.rand_scalars_np(n * t, SEED + 40 + t, bits=252).reshape(n, t, 5)
        for s in range(len(E)):                                                                 # every edge scalar, on every term in turn
            K[2 * s, s % t] = E[s]
        K[130:130 + len(E)] = E[:, None, :]                                                     # ... and on all terms of a row at once
        same = C["order_8L"][3]
        P[200:216] = same                                                                       # one order-8L point in every term
        K[208:216] = K[208:216, :1]                                                             # ... under equal scalars too
        K[214], K[215] = pm.limbs(pm.L), pm.limbs(8 * pm.L - 1)
        if t >= 2:
            for r in range(220, 250):
                p = C["decoded" if r % 2 else "order_4L"][r % CAT_N].reshape(1, 20)
                q = oracle.ed_add(p, T[1:2])
                four = np.concatenate([p, oracle.ed_neg(p), q, oracle.ed_neg(q)])
                P[r] = four[np.arange(t) % 4]
                if r < 235:
                    K[r] = K[r, 0]                                                              # equal scalars: the row sums to O (t = 2, 8)
        want = LR.oracle_lincomb(oracle, P, K)
        assert oracle.mt(oracle.ed_is_valid, P.reshape(-1, 20)).all()
        if t >= 2:
            assert PC.is_identity(oracle, want[220:235]).all() and not PC.is_identity(oracle, want[235:250]).all()
        eff = [PC.effective_scalar(pm.from_limbs(k)) for k in K[200:216].reshape(-1, 5)]       # closed form: (sum k_j) * P
        tot = np.array([pm.limbs(sum(eff[t * r:t * r + t]) % (8 * pm.L)) for r in range(16)], dtype=np.uint64)
        assert oracle.ed_eq(want[200:216], oracle.ed_scalar_mul(np.tile(same, (16, 1)), tot)).all()
        return P, K, want
    return cached(("lincomb", t), make)


@pytest.mark.parametrize("t", [1, 2, 8])
def test_ed_lincomb_same_elements(eng, oracle, t):
    P, K, want = lincomb_inputs(oracle, t)
    assert_same_elements(oracle, eng.ed_lincomb(P, K), want, ("ed_lincomb", t, "host"))
    assert_same_elements(oracle, eng.ed_lincomb(to_dev(P), to_dev(K)), want, ("ed_lincomb", t, "device"))


# ---- MSM families: (P, K, closed form or None); every family asserts what it claims to be
def edge_mixed_scalars(n, seed):
    K = V.rand_scalars_np(n, seed, bits=252)
    e = V.raw_scalar_edges(n_random=0)[: max(0, min(24, n - 8))]
    K[5:5 + len(e)] = e
    K[3] = [PC.M52] * 5
    K[4] = [1, 0, 0, 0, 0]
    return K


def torsion_sum(oracle, P, K):
    """(sum k_i j_i mod 8) * T8 for rows j_i * T8 of E[8], with the integers double_and_add walks."""
    j = PC.torsion_index(oracle, P)
    tot = sum(PC.effective_scalar(pm.from_limbs(k)) * int(i) for k, i in zip(K, j)) % 8
    return PC.torsion(oracle)[tot:tot + 1]


def family(oracle, fam, n, seed=0):
    """(P, K, want, closed): want = oracle.msm_naive_mt(P, K); closed = the family's closed form, or None."""
    def make():
        C = catalogue(oracle)
        X, names = mixed_rows(oracle)
        T = PC.torsion(oracle)
        s = SEED + 100 * fam + seed
        closed = None
        if fam == 1:                                    # one order-8L point: every bucket addition is a doubling
            P, K = np.tile(C["order_8L"][seed % CAT_N], (n, 1)), V.rand_scalars_np(n, s, bits=252)
            tot = sum(pm.from_limbs(k) for k in K) % (8 * pm.L)
            closed = oracle.ed_scalar_mul(P[:1], np.array([pm.limbs(tot)], dtype=np.uint64))
        elif fam in (2, 3):                             # P_i beside -P_i under equal scalars: computed identities everywhere
            P = tile(X, n, shift=seed)
            P[1::2] = oracle.ed_neg(P[0:2 * (n // 2):2])
            K = edge_mixed_scalars(n, s)
            K[1::2] = K[0:2 * (n // 2):2]
            if n % 2:
                K[n - 1] = 0                            # an odd row has no partner
            closed = PC.ident_rows()
            if fam == 3:                                # the last pair's scalars differ by one: a single point is left
                last = 2 * (n // 2) - 1
                K[last - 1], K[last] = pm.limbs(pm.L + 4), pm.limbs(pm.L + 5)
                closed = P[last:last + 1]
        elif fam == 4:                                  # E[8] only, plain and scaled, small scalars and the edges
            both = np.concatenate([T, PC.scale(oracle, T, s + 1)])
            P = tile(both, n, shift=seed)[np.random.default_rng(s).permutation(n)]
            K = np.zeros((n, 5), dtype=np.uint64)
            K[:, 0] = np.random.default_rng(s + 2).integers(0, 16, size=n, dtype=np.uint64)
            K[n // 2:] = tile(PC.scalars_for_torsion(), n - n // 2, shift=seed)
            closed = torsion_sum(oracle, P, K)
        elif fam == 5:                                  # decoded points under L: the sum lies in E[8] and is not O
            K = PC.scalar_rows(pm.L, n)
            for attempt in range(16):                   # (a sum in E[8] is O for one seed in eight: take the next)
                P = PC.decoded(oracle, n, s + 1000 * attempt)
                if not PC.is_identity(oracle, oracle.msm_naive_mt(P, K))[0]:
                    break
            closed = torsion_sum(oracle, PC.times_L(oracle, P), PC.scalar_rows(1, n))
        elif fam == 6:                                  # every class, identities in plain and scaled form, raw edges
            P, K = tile(X, n, shift=seed), edge_mixed_scalars(n, s)
            lam = PC.scale(oracle, PC.ident_rows(2), s + 1)
            assert not lam[:, :5].any() and np.array_equal(lam[:, 5:10], lam[:, 10:15]) and lam[0, 10:15].tolist() != pm.limbs(1)
            P[0], P[63 % n], P[64 % n], P[n - 1] = V.IDENT_ROW, lam[0], V.IDENT_ROW, lam[1]
            K[0], K[n - 1] = pm.limbs((1 << 252) - 1), pm.limbs(pm.L + 1)
            assert set(names[:min(n, len(names))]) == set(C)
        elif fam == 7:                                  # Z = 1 subgroup points, then order-8L points in scaled coordinates
            h = n // 2
            P = np.concatenate([PC.normalised(oracle, tile(C["subgroup"], h, shift=seed)), PC.scale(oracle, tile(C["order_8L"], n - h), s + 1)])
            K = edge_mixed_scalars(n, s)
            assert (P[:h, 10:15] == np.array(pm.limbs(1), dtype=np.uint64)).all() and not (P[h:, 10:15] == np.array(pm.limbs(1), dtype=np.uint64)).all(axis=1).any()
        elif fam == 8:                                  # the order-2 point only, as (0, -1, 1, 0) and (0, -l, l, 0): every window sums
            both = np.concatenate([T[4:5], PC.scale(oracle, T[4:5], s + 1)])   # to O or to (0, -1) with X = T = 0, the whole to (0, -1)
            P, K = tile(both, n), V.rand_scalars_np(n, s, bits=252)
            K[0, 0] ^= np.uint64((sum(int(k[0]) for k in K) + 1) & 1)       # an odd number of odd scalars
            closed = T[4:5]
        P, K = np.ascontiguousarray(P, dtype=np.uint64), np.ascontiguousarray(K, dtype=np.uint64)
        assert P.shape == (n, 20) and K.shape == (n, 5) and oracle.mt(oracle.ed_is_valid, P).all()
        want = oracle.msm_naive_mt(P, K)
        if closed is not None:
            assert oracle.ed_eq(want, closed)[0] == 1, ("the oracle's sum is not the closed form", fam, n)
        if fam in (2,):
            assert PC.is_identity(oracle, want)[0]
        if fam in (1, 3, 5, 8):
            assert not PC.is_identity(oracle, want)[0]
        if fam == 5:
            assert PC.order_in_e8(oracle, want) in (2, 4, 8)
        return P, K, want, closed
    return cached(("family", fam, n, seed), make)


def check_sum(oracle, got, fam_data, what):
    P, K, want, closed = fam_data
    assert_same_elements(oracle, got, want, what)
    if closed is not None:
        assert_same_elements(oracle, got, closed, (what, "closed form"))


FAMILIES = (1, 2, 3, 4, 5, 6, 7, 8)
MSM_CASES = [  # (id, n, engine knobs, test-hooks build, affine records expected (None: not asserted))
    ("257 scalar-muls + fold", 257, {}, False, None),
    ("4096 + 13 projective", 4096 + 13, {}, False, False),
    ("4096 + 13 affine", 4096 + 13, {"ZC_MSM_AFFINE": 1}, False, True),
    ("4096 + 13 run 4 window 8", 4096 + 13, {"ZC_MSM_RUN": 4, "ZC_MSM_WINDOW": 8}, True, None),
    ("4096 + 13 affine chunk 7", 4096 + 13, {"ZC_MSM_AFFINE": 1, "ZC_MSM_AFFINE_CHUNK": 7}, True, True),
    ("4096 + 13 window groups 20,10,3", 4096 + 13, {"ZC_MSM_WINDOW": 8, "ZC_MSM_GROUPS": "20,10,3"}, False, None),
]


@pytest.mark.parametrize("case", MSM_CASES, ids=[c[0] for c in MSM_CASES])
def test_msm_families(eng, oracle, case):
    _, n, knobs, hooks, affine = case

    def run(e):
        if affine is not None:
            assert bool(e.msm_plan(n)["affine"]) == affine
        if "ZC_MSM_GROUPS" in knobs:
            assert e.msm_plan(n)["window_groups"] == 3
        for fam in FAMILIES:
            data = family(oracle, fam, n)
            check_sum(oracle, e.msm(data[0], data[1]), data, ("zc_msm", case[0], "family", fam))
        data = family(oracle, 6, n)
        check_sum(oracle, e.msm(to_dev(data[0]), to_dev(data[1])), data, ("zc_msm, device", case[0]))
    if not knobs:
        return run(eng)
    with V.tuned(hooks=hooks, **knobs) as e:
        run(e)


BATCH_FAMILIES = (2, 4, 5, 6)
BATCH_CASES = [("X-1 x 7", "X-1", 7, {}), ("X x 7", "X", 7, {}), ("64 x 33 affine", 64, 33, {"ZC_MSM_AFFINE": 1})]


@pytest.mark.parametrize("case", BATCH_CASES, ids=[c[0] for c in BATCH_CASES])
def test_msm_batch_families(eng, oracle, crossover, case):
    """One family per instance, in turn, every instance with inputs of its own."""
    _, n, batch, knobs = case
    n = {"X-1": crossover - 1, "X": crossover}.get(n) or int(n)
    data = [family(oracle, BATCH_FAMILIES[b % 4], n, seed=b) for b in range(batch)]
    P, K = np.stack([d[0] for d in data]), np.stack([d[1] for d in data])

    def run(e):
        plan = e.msm_batch_plan(n, batch)
        assert plan["affine"] if knobs else plan["regime"] == ("scalar_mul" if n < crossover else "buckets")
        for form, conv in (("host", lambda a: a), ("device", to_dev)):
            got = e.msm_batch(conv(P), conv(K))
            for b in range(batch):
                check_sum(oracle, got[b], data[b], ("zc_msm_batch", case[0], form, "instance", b, "family", BATCH_FAMILIES[b % 4]))
    if not knobs:
        return run(eng)
    with V.tuned(**knobs) as e:
        run(e)


@pytest.mark.parametrize("window_bits", [0, 5, 13])
@pytest.mark.parametrize("n", [64, 257])
def test_msm_fixed_families(eng, oracle, n, window_bits):
    """Tables over families 1, 4 and 6 (the latter two hold the identity and (0, -1)); five scalar vectors per table."""
    T = PC.torsion(oracle)
    for fam in (1, 4, 6):
        P, K0, _, _ = family(oracle, fam, n)
        if fam != 1:
            idx = [PC.torsion_index(oracle, r)[0] for r in P if not r[0:5].any()]              # the x = 0 rows: O and (0, -1)
            assert 0 in idx and 4 in idx and any(np.array_equal(r, T[4]) for r in P) and any(np.array_equal(r, T[0]) for r in P)

        def make():
            small = np.zeros((n, 5), dtype=np.uint64)
            small[:, 0] = np.arange(n) % 9
            vec = np.stack([K0, PC.scalar_rows(pm.L, n), tile(PC.scalars_for_torsion(), n, shift=fam), V.rand_scalars_np(n, SEED + 60 + fam, bits=252), small])
            want = np.concatenate([oracle.msm_naive_mt(P, vec[v]) for v in range(5)])
            if fam == 4:
                for v in range(5):
                    assert oracle.ed_eq(want[v:v + 1], torsion_sum(oracle, P, vec[v]))[0] == 1
            if fam == 1:
                # L * (a point of order 8L) has order 8: n of them sum to O exactly when 8 divides n
                assert PC.order_in_e8(oracle, want[1]) is not None and bool(PC.is_identity(oracle, want[1:2])[0]) == (n % 8 == 0)
            return vec, want
        vec, want = cached(("fixed", fam, n), make)
        with eng.msm_bases(P, window_bits=window_bits) as tb:
            if window_bits:
                assert tb.plan["window_bits"] == window_bits
            assert_same_elements(oracle, tb.msm(vec), want, ("zc_msm_fixed", fam, n, window_bits, "all vectors"))
            assert_same_elements(oracle, tb.msm(to_dev(vec[2])), want[2:3], ("zc_msm_fixed", fam, n, window_bits, "device"))


# ------------------------------------------------------------------ (c) predicates and codecs, byte for byte
def codec_rows(oracle):
    """300 interleaved rows of every class, the class of each row, and whether the row lies in <B>."""
    def make():
        X, names = mixed_rows(oracle)
        even = PC.in_even_subgroup(oracle, catalogue(oracle))
        k = len(catalogue(oracle))
        member = np.array([even[names[i]][i // k] for i in range(300)])
        X, names = np.ascontiguousarray(X[:300]), names[:300]
        assert set(names[:64]) == set(catalogue(oracle))                                        # a wave holds all the classes
        return X, names, member
    return cached("codec rows", make)


def test_validity_predicates(eng, oracle):
    X, names, member = codec_rows(oracle)
    for conv in (lambda a: a, to_dev):
        assert (to_host(eng.ed_is_valid(conv(X))) == 1).all()
        got = to_host(eng.ris_is_valid(conv(X)))
        assert np.array_equal(got, oracle.mt(oracle.ris_is_valid, X))
        assert np.array_equal(got == 1, member)
    n = np.array(names)
    assert member[n == "subgroup"].all() and not member[(n == "order_2L") | (n == "order_4L") | (n == "order_8L")].any()
    assert member[n == "scaled"].any() and not member[n == "scaled"].all()
    ident = PC.is_identity(oracle, X)
    assert ident.sum() >= 2 and member[ident].all() and not member[(n == "torsion") & ~ident].any()


def test_equality_predicates(eng, oracle):
    """(P, P + T) for all eight T and (P, P in other coordinates): ed_eq is 1 only for T = O, ris_eq follows the oracle."""
    X, names, _ = codec_rows(oracle)
    T = PC.torsion(oracle)
    j = (np.arange(300) // 7) % 8                                                               # every class meets every T
    Q = oracle.mt(oracle.ed_add, X, T[j])
    S = PC.scale(oracle, X, SEED + 70)
    assert {(names[i], int(j[i])) for i in range(300)} >= {(name, t) for name in set(names) for t in range(8)}
    for conv in (lambda a: a, to_dev):
        ee = to_host(eng.ed_eq(conv(X), conv(Q)))
        assert np.array_equal(ee, oracle.mt(oracle.ed_eq, X, Q)) and np.array_equal(ee == 1, j == 0)
        re = to_host(eng.ris_eq(conv(X), conv(Q)))
        assert np.array_equal(re, oracle.mt(oracle.ris_eq, X, Q)) and (re == 1).any() and (re == 0).any() and (re[j == 0] == 1).all()
        assert (to_host(eng.ed_eq(conv(X), conv(S))) == 1).all() and oracle.mt(oracle.ed_eq, X, S).all()
        assert np.array_equal(to_host(eng.ris_eq(conv(X), conv(S))), oracle.mt(oracle.ris_eq, X, S))


def test_codecs_byte_for_byte(eng, oracle):
    X, names, _ = codec_rows(oracle)
    affine = oracle.ed_to_affine(X)
    assert affine[1].all()
    x0, y0 = ~affine[0][:, :5].any(axis=1), ~affine[0][:, 5:].any(axis=1)
    assert x0.sum() >= 4 and y0.sum() >= 4                                                      # O, (0, -1) and (+-sqrt(-1), 0), plain and scaled
    enc, ok = oracle.mt(oracle.ed_compress, X)
    assert ok.all()
    dec = oracle.mt(oracle.ed_decompress, enc)
    back = dec[1] == 1                                # the reference's decompress rejects some of its own encodings with x = 0
    assert oracle.ed_eq(dec[0][back], X[back]).all() and x0[~back].all() and back[y0].all() and back[x0].any()
    for form, conv in (("host", lambda a: a), ("device", to_dev)):
        assert_rows_equal(eng.ed_to_affine(conv(X)), affine, ("ed_to_affine", form))
        got = eng.ed_compress(conv(X))
        assert_rows_equal(got, (enc, ok), ("ed_compress", form))
        assert_rows_equal(eng.ed_decompress(got[0]), dec, ("ed_decompress", form))
        assert_rows_equal(eng.ris_compress(conv(X)), oracle.mt(oracle.ris_compress, X), ("ris_compress", form))
    # every decodable small y: the encodings small-order points arrive in
    small = np.zeros((64, 32), dtype=np.uint8)
    small[:, 0] = np.arange(64)
    small[32:, 31] = 0x80
    small[32:, 0] = np.arange(32)
    assert_rows_equal(eng.ed_decompress(small), oracle.ed_decompress(small), "ed_decompress, small y")


def test_fold_ordered(eng, oracle):
    X, _, _ = codec_rows(oracle)
    acc = X[0:1]
    for i in range(1, len(X)):
        acc = oracle.ed_add(acc, X[i:i + 1])
    assert_rows_equal(eng.ed_fold_ordered(X), acc, "ed_fold_ordered, host")
    assert_rows_equal(eng.ed_fold_ordered(to_dev(X)), acc, "ed_fold_ordered, device")
