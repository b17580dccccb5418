"""The calls and pairs of tests/test_gpu_async_scratch.py (this module holds no test).

A `Call` is one entry point at one size: how its inputs are made from a seed, how the Engine runs it on device tensors, what
the oracle says about a sample of its rows, which library-owned scratch of the context slot it reaches and the size constant
that proves it, and whether it returns before its work is done.  Sizes come from the launch thresholds of tests/entry_table.py
(each of which names the source line it mirrors), never typed in again.  `PAIRS` lists which two calls share a buffer.

Asynchrony, as read from dusk_zerocaf_amd/csrc/zerocaf_hip.hip: every row-wise entry point on device buffers (run_batched's
owner branch) and zc_msm_partial enqueue on the slot's stream and return; zc_msm, zc_msm_batch, zc_msm_fixed,
zc_msm_bases_create and zc_ris_lincomb_sum copy their result to host memory and end in hipStreamSynchronize, and so does every
call on host arrays.  A synchronous call of a pair still goes through the stream switch, but nothing can be pending behind it."""
import numpy as np

from oracle import pymodel as pm
from tests import entry_table as ET
from tests import hash_rows as HR
from tests import lincomb_rows as LR
from tests import ris_lincomb_rows as RR
from tests import ris_sum_rows as RS
from tests import scalar_ext_rows as SX
from tests import vectors as V

SEED = V.SEED + 0xA51C
SAMPLE_STEP = 2053                      # large batches: every 2053rd row and the last go to the oracle
SMALL_ROWS = 300                        # up to here every row does
FILLER_ROWS = 1 << 15                   # the strict scalar-mul that keeps stream 1 busy for about a millisecond
CORE_ROWS = 4097                        # the windowed core: 64 full waves and one row
PW_ROWS = ET.PW_MIN_ELEMS + 77          # persistent waves over the cost-sorted rows (zc_launch_plan.h PW_MIN_ELEMS)
BUCKET_N = ET.MSM_BUCKET_MIN_N          # the smallest shard of the bucket pipeline (zc_msm_plan.h MSM_BUCKET_MIN_N)
GROUPED_ENV = {"ZC_MSM_WINDOW": "8", "ZC_MSM_GROUPS": "20,10,3"}     # 33 windows in three groups: chains of the upper two on `grp`
INV_ENV = {"ZC_INV_CHUNK": "7"}
POOL = 509                              # distinct points; a prime, so that tiled rows of two seeds never line up


def sample_rows(n):
    return np.arange(n) if n <= SMALL_ROWS else np.unique(np.r_[0:n:SAMPLE_STEP, n - 1])


_pool = {}


def point_pool(oracle):
    if "P" not in _pool:
        _pool["P"] = V.base_multiples(oracle, POOL, SEED + 1)
        _pool["E"] = oracle.ris_compress(_pool["P"])
        for a in _pool.values():
            a.setflags(write=False)
    return _pool["P"], _pool["E"]


def points(oracle, count, seed):
    """count points: the pool from a seed-dependent offset, repeated"""
    P, _ = point_pool(oracle)
    return np.ascontiguousarray(P[(np.arange(count) + 37 * seed) % POOL])


def encodings(oracle, count, seed, bad_every=1001):
    """Ristretto encodings of the same, every `bad_every`-th (from row 5) undecodable"""
    _, E = point_pool(oracle)
    e = np.ascontiguousarray(E[(np.arange(count) + 37 * seed) % POOL])
    e[5::bad_every, 31] |= 0x80
    return e


def scalars(count, seed, bits=252):
    return V.rand_scalars_np(count, SEED + 100 + seed, bits=bits)


def same_group(oracle, got, want):
    LR.assert_same_points(oracle, got, want)


class Call:
    """gen(oracle, seed) -> input arrays; run(eng, dev, state) -> outputs (tensors, arrays or bytes); check(oracle, ins, outs):
    the oracle on the sampled rows of the outputs as numpy arrays; setup(eng, dev) -> state, made before anything is timed
    (a table of fixed bases).  sync: the entry point synchronises before it returns."""

    def __init__(self, id, scratch, proof, gen, run, check, sync=False, env=None, setup=None):
        self.id, self.scratch, self.proof, self.gen, self.run, self.check = id, scratch, proof, gen, run, check
        self.sync, self.env, self.setup = sync, dict(env or {}), setup


CALLS = {}


def call(*a, **kw):
    c = Call(*a, **kw)
    assert c.id not in CALLS
    CALLS[c.id] = c


# ---------------------------------------------------------------- scalar multiplications
def _gen_pk(n):
    return lambda o, s: (points(o, n, s), scalars(n, s))


def _check_strict(o, ins, outs):
    r = sample_rows(len(ins[0]))
    assert np.array_equal(outs[0][r], o.ed_scalar_mul(ins[0][r], ins[1][r]))


def _check_fast(o, ins, outs):
    r = sample_rows(len(ins[0]))
    same_group(o, outs[0][r], o.ed_scalar_mul(ins[0][r], ins[1][r]))


for _sched in (None, "unified"):
    call("strict_pw" + ("_unified" if _sched else ""), "bal", "PW_MIN_ELEMS + 77 = %d rows%s" % (PW_ROWS, ", ZC_SCHED=unified" if _sched else ""),
         _gen_pk(PW_ROWS), lambda e, d, st: (e.ed_scalar_mul(d[0], d[1]),), _check_strict, env={"ZC_SCHED": _sched} if _sched else None)
call("fast", "fast/ring", "%d rows, one 64 KB unit per wave slot" % CORE_ROWS, _gen_pk(CORE_ROWS),
     lambda e, d, st: (e.ed_scalar_mul(d[0], d[1], flags=ET.FAST),), _check_fast)


def _check_roundtrip(o, ins, outs):
    r = sample_rows(len(ins[0]))
    want, wok = o.ris_roundtrip_mul(ins[0][r], ins[1][r])
    assert np.array_equal(outs[0][r], want) and np.array_equal(outs[1][r], wok) and not outs[1][5]


call("roundtrip", "fast/ring", "%d rows, one unit per wave slot" % CORE_ROWS, lambda o, s: (encodings(o, CORE_ROWS, s), scalars(CORE_ROWS, s)),
     lambda e, d, st: e.ris_roundtrip_mul(d[0], d[1]), _check_roundtrip)


# ---------------------------------------------------------------- linear combinations per row
def _check_ed_lincomb(o, ins, outs):
    r = sample_rows(len(ins[0]))
    same_group(o, outs[0][r], LR.oracle_lincomb(o, ins[0][r], ins[1][r]))


def _check_ris_lincomb(o, ins, outs):
    r = sample_rows(len(ins[0]))
    want, wok = RR.oracle_ris_lincomb(o, ins[0][r], ins[1][r], ins[2][r])
    assert np.array_equal(outs[0][r], want) and np.array_equal(outs[1][r], wok)


for _t in (2, ET.LINCOMB_MAX_TERMS):
    call("ed_lincomb%d" % _t, "fast/ring", "%d rows, %d units per wave slot%s" % (CORE_ROWS, _t, ": the table area grows to LINCOMB_MAX_UNITS" if _t > 4 else ""),
         (lambda t: lambda o, s: (points(o, CORE_ROWS * t, s).reshape(CORE_ROWS, t, 20), scalars(CORE_ROWS * t, s).reshape(CORE_ROWS, t, 5)))(_t),
         lambda e, d, st: (e.ed_lincomb(d[0], d[1]),), _check_ed_lincomb)
for _t, _n in ((1, CORE_ROWS), (2, CORE_ROWS), (ET.LINCOMB_MAX_TERMS - 1, CORE_ROWS), (1, SMALL_ROWS)):
    call("ris_lincomb%db%s" % (_t, "" if _n == CORE_ROWS else "_%d" % _n), "fast/ring, base_table",
         "%d rows, %d terms + the base term = %d units per wave slot; the comb table of B" % (_n, _t, _t + 1),
         (lambda t, n: lambda o, s: (encodings(o, n * t, s, bad_every=97).reshape(n, t, 32), scalars(n * t, s).reshape(n, t, 5), scalars(n, s + 50)))(_t, _n),
         lambda e, d, st: e.ris_lincomb(d[0], d[1], d[2]), _check_ris_lincomb)


# ---------------------------------------------------------------- the MSM family
def _enc(o, p):
    return o.ed_compress(np.ascontiguousarray(p, dtype=np.uint64))[0]


def _check_msm(o, ins, outs):
    assert np.array_equal(_enc(o, outs[0]), _enc(o, o.msm_naive_mt(ins[0], ins[1])))


def _check_msm_batch(o, ins, outs):
    want = np.concatenate([o.msm_naive_mt(ins[0][b], ins[1][b]) for b in range(len(ins[0]))])
    assert np.array_equal(_enc(o, outs[0]), _enc(o, want))


def _check_msm_fixed(o, ins, outs):
    want = np.concatenate([o.msm_naive_mt(ins[0], ins[1][b]) for b in range(len(ins[1]))])
    assert np.array_equal(_enc(o, outs[0]), _enc(o, want))


def _check_sum(o, ins, outs):
    want, wok = RS.expected(o, ins[0], ins[1], ins[2] if len(ins) > 2 else None)
    assert outs[0].tobytes() == want and np.array_equal(outs[1], wok)


call("msm_partial", "msm, aux", "MSM_BUCKET_MIN_N = %d pairs: the bucket pipeline, normalisation forked to `aux`" % BUCKET_N, _gen_pk(BUCKET_N),
     lambda e, d, st: (e.msm_partial(d[0], d[1]),), _check_msm)
call("msm_partial_grouped", "msm, aux, grp", "6000 pairs under ZC_MSM_WINDOW=8 ZC_MSM_GROUPS=20,10,3: the chains of the two upper groups on `grp`", _gen_pk(6000),
     lambda e, d, st: (e.msm_partial(d[0], d[1]),), _check_msm, env=GROUPED_ENV)
for _n, _b in ((ET.MSM_BATCH_BUCKET_MIN_N, 33), (BUCKET_N, ET.MSM_BATCH)):
    call("msm_batch_%dx%d" % (_n, _b), "msm", "%d pairs x %d instances (ZC_MSM_BATCH_BUCKET_MIN_N = %d: buckets)" % (_n, _b, ET.MSM_BATCH_BUCKET_MIN_N),
         (lambda n, b: lambda o, s: (points(o, n * b, s).reshape(b, n, 20), scalars(n * b, s).reshape(b, n, 5)))(_n, _b),
         lambda e, d, st: (e.msm_batch(d[0], d[1]),), _check_msm_batch, sync=True)
call("msm_fixed", "msm", "257 bases, batch 5", lambda o, s: (points(o, 257, 0), scalars(257 * 5, s).reshape(5, 257, 5)),
     lambda e, d, st: (st.msm(d[1]),), _check_msm_fixed, sync=True, setup=lambda e, d: e.msm_bases(d[0]))
call("ris_sum_buckets", "ris_sum, msm, aux", "MSM_BUCKET_MIN_N + 104 = %d rows x 1 term: the bucket pipeline on the prepared pairs" % (BUCKET_N + 104),
     lambda o, s: (encodings(o, BUCKET_N + 104, s, bad_every=501).reshape(-1, 1, 32), scalars(BUCKET_N + 104, s).reshape(-1, 1, 5)),
     lambda e, d, st: e.ris_lincomb_sum(d[0], d[1]), _check_sum, sync=True)
call("ris_sum_small", "ris_sum, msm", "50 rows x 2 terms + the base term: scalar multiplications and folds in the MSM workspace",
     lambda o, s: (encodings(o, 100, s, bad_every=17).reshape(50, 2, 32), scalars(100, s).reshape(50, 2, 5), scalars(50, s + 50)),
     lambda e, d, st: e.ris_lincomb_sum(d[0], d[1], d[2]), _check_sum, sync=True)


# ---------------------------------------------------------------- the lazily built tables (300 rows)
def _k_times_base(o, k):
    return o.ed_scalar_mul(RR.basepoint_rows(len(k)), k)


def _check_wnaf(width):
    def check(o, ins, outs):
        naf = np.asarray(o.sc_compute_naf(ins[0], width)).astype(np.int64)
        k = V.limbs_array([sum(int(d) << i for i, d in enumerate(row)) % pm.L for row in naf])
        same_group(o, outs[0], _k_times_base(o, k))
    return check


call("mul_base", "base_table", "%d rows; the comb table is built by the first call of a fresh context" % SMALL_ROWS, lambda o, s: (scalars(SMALL_ROWS, s),),
     lambda e, d, st: (e.ed_mul_base(d[0]),), lambda o, ins, outs: same_group(o, outs[0], _k_times_base(o, ins[0])))
call("mul_base_compress", "base_table", "%d rows; the comb table is built by the first call of a fresh context" % SMALL_ROWS, lambda o, s: (scalars(SMALL_ROWS, s),),
     lambda e, d, st: (e.ris_mul_base_compress(d[0]),), lambda o, ins, outs: np.testing.assert_array_equal(outs[0], o.ris_compress(_k_times_base(o, ins[0]))))
call("mul_base_wnaf", "odd_table", "%d rows, width 5; the odd multiples are built by the first call of a fresh context" % SMALL_ROWS,
     lambda o, s: (V.rand_fe_np(SMALL_ROWS, SEED + 200 + s, pm.L),), lambda e, d, st: (e.ed_mul_base_wnaf(d[0], 5),), _check_wnaf(5))


# ---------------------------------------------------------------- controls: no shared scratch, results parked in the output rows
def _check_pair(fn):
    def check(o, ins, outs):
        want, wok = fn(o, ins[0])
        assert np.array_equal(outs[0], want) and np.array_equal(outs[1], wok) and 0 < wok.sum() < len(wok)
    return check


def _fe_rows(o, s):
    a = V.rand_fe_np(301, SEED + 300 + s)
    a[3::41] = 0
    return (a,)


def _sc_rows(o, s):
    a = SX.random_invert_rows(301, SEED + 310 + s)
    a[300] = 0
    return (a,)


call("fe_invert_chunked", "none (output rows)", "301 rows, ZC_INV_CHUNK=7: 43 lanes of 7 rows", _fe_rows, lambda e, d, st: e.fe_invert(d[0]),
     _check_pair(lambda o, a: o.fe_invert(a)), env=INV_ENV)
call("sc_invert_chunked", "none (output rows)", "301 rows, ZC_INV_CHUNK=7", _sc_rows, lambda e, d, st: e.sc_invert(d[0]),
     _check_pair(lambda o, a: SX.invert_expected(a)), env=INV_ENV)
call("ris_dac_chunked", "none (output rows)", "301 rows, ZC_INV_CHUNK=7", lambda o, s: (points(o, 301, s),), lambda e, d, st: (e.ris_double_and_compress(d[0]),),
     lambda o, ins, outs: np.testing.assert_array_equal(outs[0], o.ris_compress(o.ed_double(ins[0]))), env=INV_ENV)
call("sc_from_sha512", "none", "300 rows of 32 + 32 + 32 bytes", lambda o, s: tuple(HR.random_parts(300, (32, 32, 32), SEED + 320 + s)),
     lambda e, d, st: (e.sc_from_sha512(list(d), prefix=b"async"),),
     lambda o, ins, outs: np.testing.assert_array_equal(outs[0], HR.scalars_of(HR.digests(list(ins), b"async"))))

# ---------------------------------------------------------------- which two calls share a buffer
# (first, second, how the two streams are used).  "switch": the first on stream 1 behind the filler, the second under the side
# stream.  "side_first": the first under the side stream, the second at once on stream 1 -- no filler, the first call of a fresh
# context builds the table.  Every pair also runs with its calls swapped and with both calls on one stream.
PAIRS = [
    ("strict_pw", "strict_pw", "switch"),
    ("strict_pw_unified", "strict_pw_unified", "switch"),
    ("fast", "roundtrip", "switch"),
    ("roundtrip", "ed_lincomb2", "switch"),
    ("ed_lincomb2", "ris_lincomb1b", "switch"),
    ("ris_lincomb1b", "ris_lincomb7b", "switch"),
    ("fast", "ed_lincomb8", "switch"),                    # a single-unit call, then at once the call that regrows the table area
    ("ed_lincomb8", "ed_lincomb8", "switch"),
    ("msm_partial", "msm_partial", "switch"),
    ("msm_partial_grouped", "msm_partial_grouped", "switch"),
    ("msm_batch_64x33", "msm_batch_64x33", "switch"),
    ("msm_batch_4096x3", "msm_batch_4096x3", "switch"),
    ("msm_fixed", "msm_fixed", "switch"),
    ("ris_sum_buckets", "ris_sum_buckets", "switch"),
    ("ris_sum_small", "ris_sum_small", "switch"),
    ("msm_partial", "msm_batch_4096x3", "switch"),
    ("msm_batch_64x33", "msm_fixed", "switch"),
    ("ris_sum_buckets", "msm_partial", "switch"),
    ("msm_fixed", "ris_sum_small", "switch"),
    ("mul_base", "mul_base_compress", "side_first"),
    ("mul_base_wnaf", "mul_base_wnaf", "side_first"),
    ("ris_lincomb1b_300", "mul_base", "side_first"),
    ("fe_invert_chunked", "fe_invert_chunked", "switch"),
    ("sc_invert_chunked", "ris_dac_chunked", "switch"),
    ("sc_from_sha512", "sc_from_sha512", "switch"),
]
assert all(a in CALLS and b in CALLS for a, b, _ in PAIRS)
assert "msm_batch_%dx%d" % (BUCKET_N, ET.MSM_BATCH) == "msm_batch_4096x3" and ET.MSM_BATCH_BUCKET_MIN_N == 64      # the ids above name the constants' values
