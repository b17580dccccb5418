"""CPU tier: the generic step of the persistent strict scalar-mul kernel (zc_curve.hip.h: sm_g_step) after its reshaping --
no early return for a lane that is not active (its inactivity is folded into the commit predicates `add` and `dbl`), and the
result committed to Q or N inside the two branches instead of through a temporary point.

Two host builds of the very per-lane functions the kernel calls, plain and bounds-asserting:
  * tests/emul/sm_tile_emul.cpp (the one tests/test_sm_schedule_emul.py uses): whole 64-lane tiles made only of edge lanes,
    every (X:Y:Z:T) limb against the oracle's double_and_add and the step counts against tools/sm_schedule_model.py;
  * tests/emul/sm_g_step_emul.cpp: one lane step by step -- an addition leaves N alone, a doubling leaves Q alone, and a lane
    whose `active` is cleared, before its first step or after any later one, keeps Q, N and its state exactly."""
import ctypes as C
import numpy as np
import pytest

from oracle import pymodel as pm
from tests import emul_build as EB
from tests import vectors as V
from tests.test_sm_schedule_emul import model, run_tiles, tile_emul  # noqa: F401  (fixtures: the same host build)

ALL_ONES_252 = (1 << 252) - 1
ALT_10 = int("10" * 126, 2)                      # 252 bits, top bit set
ALT_01 = int("01" * 126, 2)
TRUNCATED = [7, 0, 0, 0, 8 << 48]                # a 260-bit pattern: bit 259 set, low part 7 < 2^3 -> the loop stops after 3 bits: 7 P


def edge_scalar_rows():
    vals = [0, 1, 2, 3]
    for k in (1, 31, 32, 51, 52, 251):
        vals += [1 << k, (1 << k) + 1]
    vals += [ALL_ONES_252, ALT_10, ALT_01]
    return np.array([pm.limbs(v) for v in vals] + [TRUNCATED], dtype=np.uint64)


TWO_TORSION_ROW = pm.limbs(0) + pm.limbs(pm.P - 1) + pm.limbs(1) + pm.limbs(0)          # (0, -1): order 2, passes the gate


def off_curve_row(seed):
    x, y = V.rand_fe(40, seed)[30:32]
    return np.array(pm.limbs(x) + pm.limbs(y) + pm.limbs(1) + pm.limbs(x * y % pm.P), dtype=np.uint64)      # T Z = X Y, off the curve


def edge_tile(oracle, seed):
    """64 lanes, every one an edge scalar (the 20 rows cycled, so each meets several points); lanes 20.. 23 the identity,
    24..27 the 2-torsion point, the rest multiples of the basepoint."""
    S = edge_scalar_rows()
    K = S[np.arange(64) % len(S)]
    P = V.base_multiples(oracle, 64, seed)
    P[20:24] = V.IDENT_ROW
    P[24:28] = TWO_TORSION_ROW
    K[24] = pm.limbs(ALL_ONES_252)               # the special points under a dense, an alternating and a one-bit scalar too
    K[25], K[21] = pm.limbs(ALT_10), pm.limbs(ALT_10)
    K[26], K[22] = pm.limbs(1 << 251), pm.limbs(1 << 251)
    return P, K


def test_edge_tile_every_limb_and_step_counts(tile_emul, model, oracle):
    P, K = edge_tile(oracle, V.SEED + 1600)
    vals = [pm.from_limbs(r) for r in K]
    assert pm.from_limbs(TRUNCATED) >> 259 == 1 and model.effective(pm.from_limbs(TRUNCATED)) == 7
    want = oracle.ed_scalar_mul(P, K)
    got, steps = run_tiles(tile_emul, P, K)
    assert np.array_equal(got, want)
    g, d, _ = model.tile_steps(vals, depth=1)
    assert steps[0].tolist() == [g, d, 1] and d > 100
    # lanes inactive from the first step (scalar 0: nbits = 0) end with Q = identity exactly, whatever the other lanes did
    zero = [j for j, v in enumerate(vals) if model.effective(v) == 0]
    assert zero and (got[zero] == np.array(V.IDENT_ROW, dtype=np.uint64)).all()
    # the same tile with ONE off-curve row: doubling steps off, scalar_mul_unified's schedule, still the oracle's limbs
    P[40] = off_curve_row(V.SEED + 1601)
    want = oracle.ed_scalar_mul(P, K)
    got, steps = run_tiles(tile_emul, P, K)
    assert np.array_equal(got, want)
    assert steps[0].tolist() == [max(model.cost(v) for v in vals), 0, 0]
    assert model.tile_steps(vals, depth=1, d_steps=False)[:2] == (steps[0, 0], 0)


def test_lanes_that_retire_mid_tile_keep_q(tile_emul, model, oracle):
    """One dear lane keeps the tile running for ~500 steps after the 63 others have retired (costs 0 .. 62 + popcount): every
    retired lane's Q must come out as the oracle's, i.e. untouched by the steps it sat through -- with doubling steps and,
    for an off-curve row among them, without."""
    P = V.base_multiples(oracle, 64, V.SEED + 1610)
    rng = np.random.default_rng(V.SEED + 1611)
    vals = [ALL_ONES_252] + [0] + [(int.from_bytes(rng.bytes(8), "little") % (1 << b)) | (1 << (b - 1)) for b in range(1, 63)]
    K = np.array([pm.limbs(v) for v in vals], dtype=np.uint64)
    for off in (False, True):
        if off:
            P[33] = off_curve_row(V.SEED + 1612)
        got, steps = run_tiles(tile_emul, P, K)
        assert np.array_equal(got, oracle.ed_scalar_mul(P, K))
        g, d, _ = model.tile_steps(vals, depth=1, d_steps=not off)
        assert steps[0].tolist() == [g, d, 0 if off else 1] and g + d >= 400


@pytest.fixture(scope="module", params=["plain", "checked"])
def g_step_emul(request):
    so = EB.library("sm_g_step_emul.cpp", checked=request.param == "checked")
    if so is None:
        pytest.skip("ROCm headers not present")
    lib = C.CDLL(so)
    lib.emul_g_step_keeps.restype = C.c_int
    return lib


def test_a_step_leaves_alone_what_it_must(g_step_emul, model, oracle):
    """Step by step on one lane: an addition keeps N, a doubling keeps Q, a lane with `active` cleared keeps Q, N and its
    state -- before the first step and after every later one, with and without doubling steps (additions from the stash)."""
    S = edge_scalar_rows()
    P = V.base_multiples(oracle, len(S), V.SEED + 1620)
    P[3] = V.IDENT_ROW
    P[5] = TWO_TORSION_ROW
    want = oracle.ed_scalar_mul(P, S)
    out = np.zeros(20, dtype=np.uint64)
    steps = np.zeros(2, dtype=np.int32)
    for j in range(len(S)):
        p, k = np.ascontiguousarray(P[j]), np.ascontiguousarray(S[j])
        v = pm.from_limbs(S[j])
        for use_d in (0, 1):
            bad = g_step_emul.emul_g_step_keeps(p.ctypes.data_as(C.c_void_p), k.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                                                steps.ctypes.data_as(C.c_void_p), C.c_int(use_d))
            assert bad == 0, (j, use_d)
            assert np.array_equal(out, want[j]), (j, use_d)
            g, d, _ = model.tile_steps([v], depth=1, d_steps=bool(use_d))
            assert steps[0] == g and steps[1] == 1 + 2 * g + d, (j, use_d)
    # an off-curve point never takes doubling steps in the kernel: generic steps only
    off = off_curve_row(V.SEED + 1621)
    k = np.array(pm.limbs(ALT_01), dtype=np.uint64)
    assert g_step_emul.emul_g_step_keeps(off.ctypes.data_as(C.c_void_p), k.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                                         steps.ctypes.data_as(C.c_void_p), C.c_int(0)) == 0
    assert np.array_equal(out, oracle.ed_scalar_mul(off[None, :], k[None, :])[0])
