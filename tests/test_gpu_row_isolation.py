"""GPU tier: one hostile row must not change any other row's result (tests/hostile_rows.py).

Every case runs an entry point on clean inputs, checks that result against the CPU oracle, writes patterns from the catalogue
(field elements that are 0 mod p without being five zero words, words with bits >= 2^52, off-curve and saturated point
records, undecodable bytes) over a constructed row set S, runs again and compares every output of every row outside S byte
for byte with the clean run.  Where rows share an inversion (fe_invert, fe_div, ed_to_affine, the MSM's affine normalisation) S
is built from the launch geometry and the hostile rows' own answers are checked too: the answer for the value mod p, and
out = 0 / ok = 0 where that value is 0 -- in every launch form."""
import numpy as np
import pytest

from oracle import pymodel as pm
from tests import hostile_rows as H
from tests import lincomb_rows as LR
from tests import ris_lincomb_rows as RR
from tests import vectors as V

pytestmark = pytest.mark.gpu

STRICT, LTR_BIN, BINARY_NAF, FAST = 0, 1, 2, 16
MSM_PREP_BLOCK = 64                                             # lanes per workgroup of the MSM's affine normalisation


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
    """The outputs of an Engine call as a tuple of host arrays."""
    return tuple(to_host(x) for x in (r if isinstance(r, tuple) else (r,)))


_cache = {}


def cached(key, make):
    """Clean inputs and oracle answers: computed once, shared, never written to (callers copy before planting)."""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def points(eng, n, seed):
    """n subgroup points r_i * B from the fixed-base comb (not the code under test)."""
    return cached(("points", n, seed), lambda: eng.ed_mul_base(V.rand_scalars_np(n, V.SEED + seed, bits=249)))


def scalars(n, seed, bits=252):
    return cached(("scalars", n, seed, bits), lambda: V.rand_scalars_np(n, V.SEED + seed, bits=bits))


def same_point(oracle, got, want):
    got, want = np.asarray(got).reshape(1, 20), np.asarray(want).reshape(1, 20)
    assert oracle.ed_eq(got, want)[0] == 1
    assert np.array_equal(oracle.ed_compress(got)[0], oracle.ed_compress(want)[0])
    assert np.array_equal(oracle.ris_compress(got), oracle.ris_compress(want))


def assert_equal_outputs(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        bad = np.flatnonzero((g.reshape(len(g), -1) != w.reshape(len(w), -1)).any(axis=1))
        assert len(bad) == 0, "%s: output %d differs from the oracle on rows %s" % (what, k, bad[:16])


def lane_rows(n):
    """Hostile rows for kernels that give every row its own lane: the ends, and both sides of wave and workgroup edges."""
    S = sorted({0, 1, 63, 64, 255, 256, n // 2, n - 2, n - 1})
    assert S[0] == 0 and S[-1] == n - 1 and len(S) * 10 <= n
    return S


# ------------------------------------------------------------------ (a) shared inversions
INV_SIZES = (63, 1007, 70001)
INV_CHUNKS = (1, 2, 3, 5, 16, 32, 64)
FIRST_CHUNKED = 131072 + 5                                      # the first size that chunks with default knobs (two rows per lane)


def shared_clean(eng, oracle, n):
    def make():
        D = {"den": V.rand_fe_np(n, V.SEED + 7000 + n), "num": V.rand_fe_np(n, V.SEED + 7001 + n), "pts": points(eng, n, 7002 + n)}
        D["den"][n // 2 + 1] = 0                                # a canonical zero among the clean rows
        want = {"fe_invert": oracle.mt(oracle.fe_invert, D["den"]), "fe_div": oracle.mt(oracle.fe_div, D["num"], D["den"]),
                "ed_to_affine": oracle.mt(oracle.ed_to_affine, D["pts"])}
        return D, want
    return cached(("shared", n), make)


def plant_invert(D, S, turn):
    D2 = dict(D, den=D["den"].copy())
    H.plant(D2["den"], S, H.fe_patterns(), turn)
    return D2, list(S)


def plant_div(D, S, turn):
    D2 = dict(D, den=D["den"].copy(), num=D["num"].copy())
    H.plant(D2["den"], S, H.fe_patterns(), turn)
    H.plant(D2["num"], S[::2], H.fe_patterns(), turn + 5)       # hostile numerators over hostile divisors ...
    free = [i + 1 for i in S[:-1] if i + 1 not in S]
    H.plant(D2["num"], free[:1], H.fe_patterns(), turn + 3)     # ... and one over a clean divisor: only its own quotient may change
    return D2, sorted(set(S) | set(free[:1]))


def plant_affine(D, S, turn):
    D2 = dict(D, pts=D["pts"].copy())
    H.plant(D2["pts"], S, H.point_patterns(D["pts"][5]), turn)
    return D2, list(S)


SHARED = [  # entry point, call(engine, arrays, host array -> argument), planting, turns, the row's own answer for its value
    ("fe_invert", lambda e, D, conv: e.fe_invert(conv(D["den"])), plant_invert, len(H.fe_patterns()),
     lambda D, i: H.fe_invert_model(D["den"][i])),
    ("fe_div", lambda e, D, conv: e.fe_div(conv(D["num"]), conv(D["den"])), plant_div, len(H.fe_patterns()),
     lambda D, i: H.fe_div_model(D["num"][i], D["den"][i])),
    ("ed_to_affine", lambda e, D, conv: e.ed_to_affine(conv(D["pts"])), plant_affine, len(H.point_patterns([0] * 20)),
     lambda D, i: H.ed_to_affine_model(D["pts"][i])),
]


def assert_own_answers(got, D2, rows, model, what):
    for i in rows:
        out, ok = model(D2, i)
        assert got[0][i].tolist() == [int(x) for x in out] and int(got[1][i]) == ok, (what, i, got[0][i].tolist(), int(got[1][i]))


def check_shared(e, eng, oracle, n, c):
    """Every entry point of SHARED on engine `e` (c rows per lane), host arrays on every turn and device tensors on every fourth."""
    D, want = shared_clean(eng, oracle, n)
    S = H.hostile_set(n, c)
    for name, call, plant, turns, model in SHARED:
        clean = outs(call(e, D, lambda a: a))
        assert_equal_outputs(clean, want[name], name)
        for turn in range(turns):
            D2, changed = plant(D, S, turn)
            for form, conv in (("host", lambda a: a), ("device", to_dev)):
                if form == "device" and turn % 4:
                    continue
                got = outs(call(e, D2, conv))
                what = (name, n, c, turn, form)
                H.assert_others_unchanged(clean, got, changed, what)
                assert_own_answers(got, D2, changed, model, what)


@pytest.mark.parametrize("c", INV_CHUNKS)
@pytest.mark.parametrize("n", INV_SIZES)
def test_shared_inversions(eng, oracle, n, c):
    """fe_invert, fe_div, ed_to_affine under ZC_INV_CHUNK=c: rows 0 and n - 1 and the first / middle / last / doubled
    positions of lanes that also hold clean rows carry every pattern in turn."""
    with V.tuned(ZC_INV_CHUNK=c) as e:
        check_shared(e, eng, oracle, n, c)


def test_shared_inversions_default_knobs(eng, oracle):
    """131072 + 5 rows: the first size at which the library shares inversions by itself (two rows per lane)."""
    n = FIRST_CHUNKED
    c = n // 65536
    assert c == 2
    check_shared(eng, eng, oracle, n, c)


def test_shared_inversions_in_place(eng, oracle):
    """out aliasing an input (device memory, through the C ABI: the Engine cannot alias buffers) takes the one-row kernels;
    the hostile rows get the same answers as in the chunked launch, every other row keeps the oracle's."""
    import torch
    n, c = 70001, 16
    D, want = shared_clean(eng, oracle, n)
    S = H.hostile_set(n, c)
    with V.tuned(ZC_INV_CHUNK=c) as e:
        for turn in range(0, len(H.fe_patterns()), 3):
            D2, changed = plant_div(D, S, turn)
            a, ok = to_dev(D2["den"]), torch.empty(n, dtype=torch.uint8, device="cuda")
            e._follow_torch_stream(a)
            assert e.lib.zc_fe_invert(e.ctx, a.data_ptr(), a.data_ptr(), ok.data_ptr(), n) == 0
            torch.cuda.synchronize()
            got = (to_host(a), to_host(ok))
            H.assert_others_unchanged(want["fe_invert"], got, S, ("fe_invert in place", turn))
            assert_own_answers(got, D2, S, lambda X, i: H.fe_invert_model(X["den"][i]), ("fe_invert in place", turn))
            assert_equal_outputs(outs(e.fe_invert(D2["den"])), got, "fe_invert chunked against in place")
            for alias in ("num", "den"):
                x, y = to_dev(D2["num"]), to_dev(D2["den"])
                o = x if alias == "num" else y
                assert e.lib.zc_fe_div(e.ctx, x.data_ptr(), y.data_ptr(), o.data_ptr(), ok.data_ptr(), n) == 0
                torch.cuda.synchronize()
                got = (to_host(o), to_host(ok))
                H.assert_others_unchanged(want["fe_div"], got, changed, ("fe_div in place", alias, turn))
                assert_own_answers(got, D2, changed, lambda X, i: H.fe_div_model(X["num"][i], X["den"][i]), ("fe_div in place", alias, turn))
            assert_equal_outputs(outs(e.fe_div(D2["num"], D2["den"])), got, "fe_div chunked against in place")


# ------------------------------------------------------------------ (b) one lane per row
def enc_of(eng, P, ristretto):
    return eng.ris_compress(P) if ristretto else eng.ed_compress(P)[0]


def bytes_patterns(oracle, ristretto):
    return cached(("undecodable", ristretto), lambda: H.undecodable(oracle.ris_decompress if ristretto else oracle.ed_decompress))


def lane_inputs(eng, n, seed):
    P, Q = points(eng, n, seed), points(eng, n, seed + 1).copy()
    Q[::2] = P[::2]                                             # equal and unequal pairs
    return {"P": P, "Q": Q, "K": scalars(n, seed + 2)}


def pt_call(name, *keys, **kw):
    return lambda e, I: getattr(e, name)(*[I[k] for k in keys], **kw)


def pt_want(name, *keys, extra=()):
    """check(oracle, outputs, inputs): every output equals the oracle's `name` on the same inputs."""
    def check(o, got, I):
        w = o.mt(getattr(o, name), *[I[k] for k in keys], extra=extra)
        assert_equal_outputs(got, w if isinstance(w, tuple) else (w,), name)
    return check


def same_elements(oracle, got, I):
    """The windowed core: the group elements of Mul<Scalar>, not its limbs."""
    LR.assert_same_points(oracle, got[0], oracle.mt(oracle.ed_scalar_mul, I["P"], I["K"]))


N_LANE = 4097 + 300
PER_LANE = [  # (id, n, call(engine, inputs), check(oracle, outputs of the clean run, inputs), planted inputs)
    ("ed_compress", N_LANE, pt_call("ed_compress", "P"), pt_want("ed_compress", "P"), ("P",)),
    ("ed_is_valid", N_LANE, pt_call("ed_is_valid", "P"), pt_want("ed_is_valid", "P"), ("P",)),
    ("ed_eq", N_LANE, pt_call("ed_eq", "P", "Q"), pt_want("ed_eq", "P", "Q"), ("P", "Q")),
    ("ris_eq", N_LANE, pt_call("ris_eq", "P", "Q"), pt_want("ris_eq", "P", "Q"), ("P", "Q")),
    ("ris_compress", N_LANE, pt_call("ris_compress", "P"), pt_want("ris_compress", "P"), ("P",)),
    ("ris_is_valid", N_LANE, pt_call("ris_is_valid", "P"), pt_want("ris_is_valid", "P"), ("P",)),
    ("ed_coset4", N_LANE, pt_call("ed_coset4", "P"), pt_want("ed_coset4", "P"), ("P",)),
    ("ed_mul_by_pow_2", N_LANE, lambda e, I: e.ed_mul_by_pow_2(I["P"], 5), pt_want("ed_mul_by_pow_2", "P", extra=(5,)), ("P",)),
    ("ed_add", N_LANE, pt_call("ed_add", "P", "Q"), pt_want("ed_add", "P", "Q"), ("P", "Q")),
    ("ed_sub", N_LANE, pt_call("ed_sub", "P", "Q"), pt_want("ed_sub", "P", "Q"), ("P", "Q")),
    ("ed_double", N_LANE, pt_call("ed_double", "P"), pt_want("ed_double", "P"), ("P",)),
    ("ed_neg", N_LANE, pt_call("ed_neg", "P"), pt_want("ed_neg", "P"), ("P",)),
    ("ed_scalar_mul strict 1000", 1000, pt_call("ed_scalar_mul", "P", "K"), pt_want("ed_scalar_mul", "P", "K"), ("P",)),
    ("ed_scalar_mul strict 2^14 + 1", (1 << 14) + 1, pt_call("ed_scalar_mul", "P", "K"), pt_want("ed_scalar_mul", "P", "K"), ("P",)),
    ("ed_scalar_mul fast", 2048 + 5, pt_call("ed_scalar_mul", "P", "K", flags=FAST), same_elements, ("P",)),
]


def run_isolation(eng, oracle, what, I, call, check, planted, patterns, S):
    """The harness: clean run against the oracle, then every pattern in turn over S; rows outside S must not change."""
    clean = outs(call(eng, I))
    check(oracle, clean, I)
    for turn in range(-(-len(patterns) // len(S))):
        I2 = dict(I)
        for j, key in enumerate(planted):
            I2[key] = I[key].copy()
            H.plant(I2[key], S if j == 0 else S[1::2], patterns, turn * len(S) + 3 * j)
        H.assert_others_unchanged(clean, outs(call(eng, I2)), S, (what, turn))


@pytest.mark.parametrize("case", PER_LANE, ids=[c[0] for c in PER_LANE])
def test_per_lane_kernels(eng, oracle, case):
    what, n, call, check, planted = case
    I = lane_inputs(eng, n, 7100 + n)
    run_isolation(eng, oracle, what, I, call, check, planted, H.point_patterns(I["P"][5]), lane_rows(n))


@pytest.mark.parametrize("ristretto", [False, True], ids=["ed_decompress", "ris_decompress"])
def test_decoders_on_hostile_bytes(eng, oracle, ristretto):
    n = N_LANE
    I = {"E": cached(("enc", n, ristretto), lambda: enc_of(eng, points(eng, n, 7200), ristretto))}
    name = "ris_decompress" if ristretto else "ed_decompress"
    run_isolation(eng, oracle, name, I, pt_call(name, "E"), pt_want(name, "E"), ("E",), bytes_patterns(oracle, ristretto), lane_rows(n))


def test_ris_roundtrip_mul_on_hostile_bytes(eng, oracle):
    n = 2048 + 5
    I = {"E": cached(("enc", n, True), lambda: enc_of(eng, points(eng, n, 7200), True)), "K": scalars(n, 7201)}
    run_isolation(eng, oracle, "ris_roundtrip_mul", I, pt_call("ris_roundtrip_mul", "E", "K"), pt_want("ris_roundtrip_mul", "E", "K"), ("E",),
                  bytes_patterns(oracle, True), lane_rows(n))


# ------------------------------------------------------------------ (c) - (e) MSM: hostile points under zero scalars
def prep_stride(cnt, ac):
    """Rows cnt apart by this stride share a lane of the affine normalisation at ac points per lane."""
    lanes = -(-cnt // ac)
    return MSM_PREP_BLOCK * -(-lanes // MSM_PREP_BLOCK)


def msm_hostile_rows(cnt, ac, extra=()):
    """ac = 0: projective records (a lane per point)."""
    S = set(H.hostile_set(cnt, ac, prep_stride(cnt, ac)) if ac else [0, cnt - 1]) | {cnt // 3, 2 * cnt // 3} | set(extra)
    S = sorted(S)
    H.check_hostile_set(S, cnt, max(ac, 1), prep_stride(cnt, ac) if ac else None)
    return S


def msm_scalars(n, seed):
    def make():
        K = V.rand_scalars_np(n, V.SEED + seed, bits=252)
        e = V.raw_scalar_edges(n_random=0)[: max(0, min(24, n - 8))]
        K[5:5 + len(e)] = e
        K[3] = [(1 << 52) - 1] * 5
        K[4] = [1, 0, 0, 0, 0]
        return K
    return cached(("msm scalars", n, seed), make)


def check_msm(e, eng, oracle, n, ac, affine):
    if n >= 4096:
        assert bool(e.msm_plan(n)["affine"]) == affine
    P = points(eng, n, 7300 + n)
    S = msm_hostile_rows(n, ac)
    K = msm_scalars(n, 7301).copy()
    K[S] = 0
    pats = H.point_patterns(P[5])
    first = None
    for turn in range(-(-len(pats) // len(S))):
        P2 = P.copy()
        H.plant(P2, S, pats, turn * len(S))
        got = e.msm(P2, K)
        if first is None:
            first = got
            same_point(oracle, got, oracle.msm_naive_mt(P2, K))     # `&P * &0` is the identity whatever P holds: later turns have this sum too
        else:
            same_point(oracle, got, first)


MSM_CASES = [  # (id, n, engine knobs, test-hooks build, points per lane of the normalisation (0: projective records))
    ("257 scalar-muls + fold", 257, {}, False, 0),
    ("4096 + 13 projective", 4096 + 13, {}, False, 0),
    ("4096 + 13 affine", 4096 + 13, {"ZC_MSM_AFFINE": 1}, False, 1),
    ("4096 + 13 affine chunk 1", 4096 + 13, {"ZC_MSM_AFFINE": 1, "ZC_MSM_AFFINE_CHUNK": 1}, True, 1),
    ("4096 + 13 affine chunk 2", 4096 + 13, {"ZC_MSM_AFFINE": 1, "ZC_MSM_AFFINE_CHUNK": 2}, True, 2),
    ("4096 + 13 affine chunk 7", 4096 + 13, {"ZC_MSM_AFFINE": 1, "ZC_MSM_AFFINE_CHUNK": 7}, True, 7),
    ("2^17 + 77 default", (1 << 17) + 77, {}, False, 1),
]


@pytest.mark.parametrize("case", MSM_CASES, ids=[c[0] for c in MSM_CASES])
def test_msm_hostile_points_under_zero_scalars(eng, oracle, case):
    _, n, knobs, hooks, ac = case
    if not knobs:
        return check_msm(eng, eng, oracle, n, ac, ac > 0)
    with V.tuned(hooks=hooks, **knobs) as e:
        check_msm(e, eng, oracle, n, ac, True)


def batch_rows(n, batch, ac):
    """Flat hostile rows of a batch: two pairs of every instance (pairs b and n - 1 - b of instance b, so that they do not
    line up in the lanes of the normalisation, whose stride is a multiple of 64), and the rows the lanes call for."""
    return msm_hostile_rows(n * batch, ac, extra=[b * n + b % n for b in range(batch)] + [b * n + n - 1 - b % n for b in range(batch)])


def check_msm_batch(e, eng, oracle, n, batch, ac):
    P = points(eng, n * batch, 7400 + n).reshape(batch, n, 20)
    K = msm_scalars(n * batch, 7401).copy()
    S = batch_rows(n, batch, ac)
    K[S] = 0
    K = K.reshape(batch, n, 5)
    pats = H.point_patterns(P[0, 5])
    # hostile points under zero scalars as padding in every instance
    first = None
    for turn in range(-(-len(pats) // len(S))):
        P2 = P.copy()
        H.plant(P2.reshape(-1, 20), S, pats, turn * len(S))
        got = e.msm_batch(P2, K)
        if first is None:
            first = got
            for b in range(batch):
                same_point(oracle, got[b], oracle.msm_naive_mt(P2[b], K[b]))
        else:
            LR.assert_same_points(oracle, got, first)
    # one instance wholly hostile, its scalars as they are: the others keep the limbs of the clean run
    clean = e.msm_batch(P, K)
    LR.assert_same_points(oracle, clean, first)
    bad = batch // 2
    rows = [b for b in range(batch) if b != bad]
    assert K[bad].any(axis=1).sum() >= n - 8
    for turn in range(2):
        P2 = P.copy()
        H.plant(P2[bad], list(range(n)), pats, turn * 7)
        got = e.msm_batch(P2, K)
        assert np.array_equal(got[rows], clean[rows]), ("instances changed by a hostile one", np.flatnonzero((got != clean).any(axis=1)))


BATCH_CASES = [  # (id, n, batch, knobs, test-hooks build, points per lane)
    ("X-1 x 7", "X-1", 7, {}, False, 0),
    ("X x 7", "X", 7, {}, False, 0),
    ("64 x 33 affine", 64, 33, {"ZC_MSM_AFFINE": 1}, False, 1),
    ("64 x 33 affine chunk 7", 64, 33, {"ZC_MSM_AFFINE": 1, "ZC_MSM_AFFINE_CHUNK": 7}, True, 7),
    ("4096 x 40", 4096, 40, {}, False, 1),
]


@pytest.mark.parametrize("case", BATCH_CASES, ids=[c[0] for c in BATCH_CASES])
def test_msm_batch_hostile_instances(eng, oracle, crossover, case):
    _, n, batch, knobs, hooks, ac = case
    n = {"X-1": crossover - 1, "X": crossover}.get(n) or int(n)
    if not knobs:
        if ac:
            assert eng.msm_batch_plan(n, batch)["affine"]
        return check_msm_batch(eng, eng, oracle, n, batch, ac)
    with V.tuned(hooks=hooks, **knobs) as e:
        assert e.msm_batch_plan(n, batch)["affine"]
        check_msm_batch(e, eng, oracle, n, batch, ac)


FIXED_CASES = [(n, ac) for n in (64, 257) for ac in (1, 2, 7)]


@pytest.mark.parametrize("n,ac", FIXED_CASES)
def test_msm_fixed_hostile_bases(eng, oracle, n, ac):
    """A table over n bases with hostile ones at S (ac = 1: the product library; 2, 7: ZC_MSM_AFFINE_CHUNK on the test-hooks
    build shares each lane's inversion among that many bases), five scalar vectors that are zero at S."""
    P = points(eng, n, 7500 + n)
    S = msm_hostile_rows(n, ac)
    K = msm_scalars(5 * n, 7501).copy().reshape(5, n, 5)
    K[:, S] = 0
    pats = H.point_patterns(P[5])
    with V.tuned(hooks=ac > 1, ZC_MSM_AFFINE_CHUNK=ac if ac > 1 else None) as e:
        first = None
        for turn in range(-(-len(pats) // len(S))):
            P2 = P.copy()
            H.plant(P2, S, pats, turn * len(S))
            with e.msm_bases(P2) as tb:
                got = tb.msm(K)
            if first is None:
                first = got
                for v in range(5):
                    same_point(oracle, got[v], oracle.msm_naive_mt(P2, K[v]))
            else:
                LR.assert_same_points(oracle, got, first)


# ------------------------------------------------------------------ (f) linear combinations per row
LINCOMB_SIZES = (257, (1 << 14) + 5)


def lincomb_rows(n):
    S = sorted({0, 1, 63, 64, 127, 128, n // 2, n - 2, n - 1})
    assert len(S) * 10 <= n
    return S


@pytest.mark.parametrize("n", LINCOMB_SIZES)
@pytest.mark.parametrize("t", [1, 2, 8])
def test_ed_lincomb_hostile_terms(eng, oracle, t, n):
    P = points(eng, n * t, 7600 + t).reshape(n, t, 20)
    K = scalars(n * t, 7601 + t).reshape(n, t, 5).copy()
    S = lincomb_rows(n)
    term = {i: j % t for j, i in enumerate(S)}
    for i, j in term.items():
        K[i, j] = 0                                             # the hostile term of row i sits under a zero scalar
    want = cached(("lincomb", n, t), lambda: LR.oracle_lincomb(oracle, P, K))
    clean = eng.ed_lincomb(P, K)
    LR.assert_same_points(oracle, clean, want)
    pats = H.point_patterns(P[0, 0])
    for turn in range(-(-len(pats) // len(S))):
        P2 = P.copy()
        for j, i in enumerate(S):
            P2[i, term[i]] = np.array(pats[(j + turn * len(S)) % len(pats)][1], dtype=np.uint64)
        got = eng.ed_lincomb(P2, K)
        H.assert_others_unchanged(clean, got, S, ("ed_lincomb", t, n, turn))
        LR.assert_same_points(oracle, got[S], LR.oracle_lincomb(oracle, P2[S], K[S]))   # the oracle's rows over the same arrays
    # wholly hostile rows, scalars as they are
    K3 = scalars(n * t, 7601 + t).reshape(n, t, 5)
    clean = eng.ed_lincomb(P, K3)
    P2 = P.copy()
    for j, i in enumerate(S):
        for k in range(t):
            P2[i, k] = np.array(pats[(j + 5 * k) % len(pats)][1], dtype=np.uint64)
    H.assert_others_unchanged(clean, eng.ed_lincomb(P2, K3), S, ("ed_lincomb, hostile rows", t, n))


@pytest.mark.parametrize("n", LINCOMB_SIZES)
@pytest.mark.parametrize("base", [True, False], ids=["base term", "no base term"])
def test_ris_lincomb_hostile_terms(eng, oracle, base, n):
    t = 2
    E = enc_of(eng, points(eng, n * t, 7700), True).reshape(n, t, 32)
    K = scalars(n * t, 7701).reshape(n, t, 5).copy()
    KB = scalars(n, 7702) if base else None
    S = lincomb_rows(n)
    for j, i in enumerate(S):
        K[i, j % t] = 0
    want = cached(("ris lincomb", n, base), lambda: RR.oracle_ris_lincomb(oracle, E, K, KB))
    clean = outs(eng.ris_lincomb(E, K, KB))
    RR.assert_same_bytes(clean, want)
    assert clean[1].all()
    pats = bytes_patterns(oracle, True)
    for turn in range(len(pats)):
        E2 = E.copy()
        for j, i in enumerate(S):
            E2[i, j % t] = pats[(j + turn) % len(pats)][1]
        got = outs(eng.ris_lincomb(E2, K, KB))
        H.assert_others_unchanged(clean, got, S, ("ris_lincomb", base, n, turn))
        assert not got[1][S].any() and not got[0][S].any()      # an undecodable term: ok = 0 and zero bytes, also under a zero scalar
        RR.assert_same_bytes((got[0][S], got[1][S]), RR.oracle_ris_lincomb(oracle, E2[S], K[S], None if KB is None else KB[S]))
    K3 = scalars(n * t, 7701).reshape(n, t, 5)
    clean = outs(eng.ris_lincomb(E, K3, KB))
    E2 = E.copy()
    for j, i in enumerate(S):
        E2[i, :] = np.stack([pats[(j + k) % len(pats)][1] for k in range(t)])
    got = outs(eng.ris_lincomb(E2, K3, KB))
    H.assert_others_unchanged(clean, got, S, ("ris_lincomb, hostile rows", base, n))
    assert not got[1][S].any() and not got[0][S].any()


# ------------------------------------------------------------------ (g) limb bits >= 2^52 of a scalar are ignored
def junk_above_52(K, seed):
    rng = np.random.default_rng(V.SEED + seed)
    junk = rng.integers(1, 1 << 12, size=K.shape, dtype=np.uint64) << np.uint64(52)
    J = K | junk
    assert ((J >> np.uint64(52)) != 0).all() and np.array_equal(J & np.uint64(H.M52), K)
    return J


def test_scalar_bits_above_2_52_are_ignored(eng, oracle):
    """Every Mul<Scalar> operand: random junk OR-ed into bits 52..63 of every word changes no output byte, and the output for
    the masked words is the oracle's."""
    n = 300
    P = points(eng, n, 7800)
    base = RR.basepoint_rows(n)
    K = scalars(n, 7801).copy()
    edges = V.raw_scalar_edges()
    K[:len(edges)] = edges
    K[len(edges)] = 0
    K[len(edges) + 1] = pm.limbs(pm.L)
    Kc = scalars(n, 7802, bits=249).copy()                      # canonical scalars for the two left-to-right variants
    Kc[0], Kc[1], Kc[2] = 0, [1, 0, 0, 0, 0], pm.limbs(pm.L - 1)
    J, Jc = junk_above_52(K, 7803), junk_above_52(Kc, 7804)
    strict = oracle.mt(oracle.ed_scalar_mul, P, K)

    def same(a, b, what):
        a, b = outs(a), outs(b)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), what
        return a

    got = same(eng.ed_scalar_mul(P, J), eng.ed_scalar_mul(P, K), "strict")
    assert np.array_equal(got[0], strict)
    for mode in (LTR_BIN, BINARY_NAF):
        got = same(eng.ed_scalar_mul(P, Jc, flags=mode), eng.ed_scalar_mul(P, Kc, flags=mode), mode)
        assert np.array_equal(got[0], oracle.mt(oracle.ed_scalar_mul_mode, P, Kc, extra=(mode,)))
    got = same(eng.ed_scalar_mul(P, J, flags=FAST), eng.ed_scalar_mul(P, K, flags=FAST), "fast")
    LR.assert_same_points(oracle, got[0], strict)
    P3 = np.ascontiguousarray(P[:, :15])
    got = same(eng.proj_scalar_mul(P3, J), eng.proj_scalar_mul(P3, K), "proj_scalar_mul")
    assert np.array_equal(got[0], oracle.mt(oracle.proj_scalar_mul, P3, K))
    kb = oracle.mt(oracle.ed_scalar_mul, base, K)
    got = same(eng.ed_mul_base(J), eng.ed_mul_base(K), "ed_mul_base")
    LR.assert_same_points(oracle, got[0], kb)
    got = same(eng.ris_mul_base_compress(J), eng.ris_mul_base_compress(K), "ris_mul_base_compress")
    assert np.array_equal(got[0], oracle.mt(oracle.ris_compress, kb))
    E = enc_of(eng, P, True)
    got = same(eng.ris_roundtrip_mul(E, J), eng.ris_roundtrip_mul(E, K), "ris_roundtrip_mul")
    assert_equal_outputs(got, oracle.mt(oracle.ris_roundtrip_mul, E, K), "ris_roundtrip_mul")
    got = same(eng.msm(P, J), eng.msm(P, K), "msm")
    same_point(oracle, got[0], oracle.msm_naive_mt(P, K))
    P2, K2, J2 = P.reshape(n // 2, 2, 20), K.reshape(n // 2, 2, 5), J.reshape(n // 2, 2, 5)
    got = same(eng.ed_lincomb(P2, J2), eng.ed_lincomb(P2, K2), "ed_lincomb")
    LR.assert_same_points(oracle, got[0], LR.oracle_lincomb(oracle, P2, K2))
    E2, KB, JB = E.reshape(n // 2, 2, 32), Kc[:n // 2], Jc[:n // 2]
    got = same(eng.ris_lincomb(E2, J2, JB), eng.ris_lincomb(E2, K2, KB), "ris_lincomb")
    RR.assert_same_bytes(got, RR.oracle_ris_lincomb(oracle, E2, K2, KB))
