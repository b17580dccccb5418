"""GPU tier: what a context owns over its life -- staging buffers, the MSM workspace, the lazily built tables, the table ring,
streams and events -- is created on first use, regrown when a call needs more, and returned when the context closes.
Expected values come from the CPU oracle, computed once for the module."""
import numpy as np
import pytest

from tests import ris_lincomb_rows as RR
from tests import vectors as V

pytestmark = pytest.mark.gpu

FAST = 16
PW_MIN_ELEMS = 1 << 17              # strict scalar-mul batches from here on sort their lanes by cost: the balance buffer
MSM_BUCKET_MIN_N = 4096             # zc_msm shards from here on take the bucket pipeline, smaller ones scalar-muls + folds
SLACK = 8 << 20                     # free-memory noise allowed across create / close cycles (as tests/test_gpu_msm_fixed.py)


@pytest.fixture(scope="module")
def ref(oracle):
    """Inputs and the oracle's answers, shared by the tests below and left unchanged by them."""
    r = {}
    base = RR.basepoint_rows
    pool = V.base_multiples(oracle, 1024, V.SEED + 900)
    r["pool"] = pool
    # MSM: 2^14 pairs over the pool; the sums of the first 100, 4096 and all of them
    r["P"] = np.tile(pool, (16, 1))
    r["K"] = V.rand_scalars_np(1 << 14, V.SEED + 901, bits=252)
    r["msm"] = {n: oracle.msm_naive_mt(r["P"][:n], r["K"][:n]) for n in (100, MSM_BUCKET_MIN_N, 1 << 14)}
    # strict scalar-mul at the balance threshold: every 2053rd row against the oracle, limb for limb
    r["SP"] = np.tile(pool, (PW_MIN_ELEMS // 1024, 1))
    r["SK"] = V.rand_scalars_np(PW_MIN_ELEMS, V.SEED + 902, bits=252)
    r["rows"] = np.arange(0, PW_MIN_ELEMS, 2053)
    r["strict"] = oracle.mt(oracle.ed_scalar_mul, r["SP"][r["rows"]], r["SK"][r["rows"]])
    # wire-format linear combination: 3 rows of 2 terms and a basepoint term
    r["E"] = np.ascontiguousarray(oracle.ris_compress(pool[:6]).reshape(3, 2, 32))
    r["LK"] = V.rand_scalars_np(6, V.SEED + 903, bits=252).reshape(3, 2, 5)
    r["LB"] = V.rand_scalars_np(3, V.SEED + 904, bits=252)
    r["lincomb"] = RR.oracle_ris_lincomb(oracle, r["E"], r["LK"], r["LB"])
    # ordered fold of three points
    r["fold"] = oracle.ed_add(oracle.ed_add(pool[0:1], pool[1:2]), pool[2:3])
    # multiples of the basepoint: 3 scalars for the w-NAF, 65 for the comb and the windowed core
    r["BK"] = V.rand_scalars_np(65, V.SEED + 905, bits=249)
    r["kB"] = oracle.ed_scalar_mul(base(65), r["BK"])
    r["FP"] = pool[:65]
    r["fast"] = oracle.ed_scalar_mul(r["FP"], r["BK"])
    # field products at 1000 and 2^16 rows
    r["a"], r["b"] = V.rand_fe_np(1 << 16, V.SEED + 906), V.rand_fe_np(1 << 16, V.SEED + 907)
    r["ab"] = oracle.mt(oracle.fe_mul, r["a"], r["b"])
    return r


def same_point(oracle, got, want):
    """The same group element with the same encodings (not the same limbs)."""
    got, want = np.asarray(got), np.asarray(want)
    assert oracle.ed_eq(got, want).all()
    assert np.array_equal(oracle.ed_compress(got)[0], oracle.ed_compress(want)[0])
    assert np.array_equal(oracle.ris_compress(got), oracle.ris_compress(want))


def check_msm(e, oracle, ref, n):
    same_point(oracle, e.msm(ref["P"][:n], ref["K"][:n]), ref["msm"][n])


def check_wnaf(e, oracle, ref):
    same_point(oracle, e.ed_mul_base_wnaf(ref["BK"][:3], 5), ref["kB"][:3])


def exercise(e, oracle, ref, small_only=False):
    """Every resource a context creates lazily, touched once, at the smallest size that reaches it.  Returns the fixed-base
    table it leaves LIVE (the context's close must take it along)."""
    # five staging buffers, the comb table, the table ring with its state and its error word
    RR.assert_same_bytes(e.ris_lincomb(ref["E"], ref["LK"], ref["LB"]), ref["lincomb"])
    # scalar-muls + folds in the MSM workspace
    check_msm(e, oracle, ref, 100)
    # the exchange buffer (host points are folded there)
    assert np.array_equal(e.ed_fold_ordered(ref["pool"][:3]), ref["fold"])
    # the odd-multiples table
    check_wnaf(e, oracle, ref)
    if not small_only:
        # the balance buffer (balance_index is reached from strict batches of PW_MIN_ELEMS rows only)
        got = e.ed_scalar_mul(ref["SP"], ref["SK"])
        assert np.array_equal(got[ref["rows"]], ref["strict"])
        # the bucket pipeline: the workspace regrown, the side streams and their events
        check_msm(e, oracle, ref, MSM_BUCKET_MIN_N)
    # a fixed-base table of at least 1 MiB (its allocation is exact; every buffer above is at least 1 MiB through grow's floor)
    assert e.msm_fixed_plan(1024)["table_mib"] >= 1
    return e.msm_bases(ref["pool"])


def cycle(oracle, ref):
    import dusk_zerocaf_amd as z
    e = z.Engine()
    try:
        tb = exercise(e, oracle, ref)
    finally:
        e.close()                                  # with the table live
    tb.id = 0


def test_context_cycles_return_all_device_memory(oracle, ref):
    """Ten create / exercise / close cycles: after the first (which warms the runtime's own pools) free device memory stays
    within 8 MiB.  Every buffer of `exercise` holds at least 1 MiB, so over the nine measured cycles a single one that
    close forgot would show.  Objects smaller than that -- events, streams, the 17 KB ring state, the pinned error word --
    cannot be seen this way and are not covered here.  Every cycle also checks the n = 100 MSM and the w-NAF rows against
    the oracle: a re-created context computes correctly."""
    import torch
    cycle(oracle, ref)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(9):
        cycle(oracle, ref)
    torch.cuda.synchronize()
    drift = torch.cuda.mem_get_info()[0] - free0
    print("free-memory drift over 9 cycles: %d bytes" % drift)
    assert abs(drift) < SLACK


def test_buffers_regrow_between_calls(oracle, ref):
    """Staging buffers and the MSM workspace are reallocated when a call needs more than they hold, and serve the smaller
    calls after it: 2^16 rows of 40 bytes exceed the 1 MiB floor of the staging buffers; the workspace grows from the
    scalar-mul + fold path (n = 100) through two bucket plans and then serves the small path again."""
    import dusk_zerocaf_amd as z
    e = z.Engine()
    try:
        for n in (1000, 1 << 16, 1000):
            assert np.array_equal(e.fe_mul(ref["a"][:n], ref["b"][:n]), ref["ab"][:n]), n
        for n in (100, MSM_BUCKET_MIN_N, 1 << 14, 100):
            check_msm(e, oracle, ref, n)
    finally:
        e.close()


def test_contexts_are_independent(oracle, ref):
    """Two contexts build their own tables and ring; closing one leaves the other's intact."""
    import dusk_zerocaf_amd as z
    first, second = z.Engine(), z.Engine()
    tables = []
    try:
        tables = [exercise(e, oracle, ref, small_only=True) for e in (first, second)]
        first.close()
        tables[0].id = 0
        same_point(oracle, second.ed_mul_base(ref["BK"]), ref["kB"])                              # its comb table
        check_wnaf(second, oracle, ref)                                                            # its odd multiples
        same_point(oracle, second.ed_scalar_mul(ref["FP"], ref["BK"], flags=FAST), ref["fast"])    # its ring
    finally:
        first.close()
        second.close()
        for t in tables:
            t.id = 0
