"""CPU tier: the tile loop of the persistent strict scalar-mul kernel (k_ed_scalar_mul_pw) on 64 real lanes.

tests/emul/sm_tile_emul.cpp drives the very per-lane functions the kernel calls (zc_curve.hip.h: sm_lane, sm_g_step,
sm_d_step, ptm_double_valid and its validity gate) with every ballot written as a loop over the lanes, so the schedule --
generic steps alternating with wave-uniform doubling steps, one stashed addend per lane -- is checked limb for limb against
the oracle before any GPU time is spent, in the plain, the bounds-asserting and (ZC_EMUL_SANITIZE) the sanitizer build.
The step counts must be those of tools/sm_schedule_model.py: the model and the kernel are the same schedule."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pymodel as pm
from tests import emul_build as EB
from tests import vectors as V
from tests.emul_build import EMUL_DIR, ROOT


@pytest.fixture(scope="module", params=["plain", "checked"])
def tile_emul(request):
    checked = request.param == "checked"
    so = EB.library("sm_tile_emul.cpp", checked=checked, sanitize=bool(os.environ.get("ZC_EMUL_SANITIZE")))
    if so is None:
        pytest.skip("ROCm headers not present")
    return C.CDLL(so)


@pytest.fixture(scope="module")
def model():
    spec = importlib.util.spec_from_file_location("sm_schedule_model", os.path.join(ROOT, "tools", "sm_schedule_model.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def run_tiles(lib, P, K, allow_d=1):
    P, K = np.ascontiguousarray(P, dtype=np.uint64), np.ascontiguousarray(K, dtype=np.uint64)
    n = len(P)
    out = np.zeros_like(P)
    steps = np.zeros(((n + 63) // 64, 3), dtype=np.int32)
    lib.emul_sm_tiles(P.ctypes.data_as(C.c_void_p), K.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.c_size_t(n),
                      steps.ctypes.data_as(C.c_void_p), C.c_int(allow_d))
    return out, steps


def edge_scalar_rows():
    return [[0] * 5, [1, 0, 0, 0, 0], pm.limbs(pm.L), pm.limbs(pm.L - 1), pm.limbs(2**249 - 1), [(1 << 52) - 1] * 5,
            [0, 0, 0, 0, 1 << 47], pm.limbs(8), pm.limbs(2**248), pm.limbs(3), pm.limbs(2), pm.limbs((1 << 252) - 1)]


def invalid_rows(oracle, seed):
    """(off the curve with T Z = X Y, on the curve with T Z != X Y, Z = 0 from a valid point, the all-zero row,
    a valid point with every coordinate's limbs raised by p)."""
    G = V.base_multiples(oracle, 5, seed)
    x, y = V.rand_fe(40, seed + 1)[30:32]
    off = np.array(pm.limbs(x) + pm.limbs(y) + pm.limbs(1) + pm.limbs(x * y % pm.P), dtype=np.uint64)
    badt = G[1].copy()
    badt[15:20] = oracle.fe_neg(G[1:2, 15:20])[0]                                    # T -> -T: the curve identity holds, T Z = -X Y
    z0 = G[2].copy()
    z0[10:15] = 0
    zero = np.zeros(20, dtype=np.uint64)
    big = np.array(sum([pm.limbs(pm.from_limbs(G[3, 5 * c:5 * c + 5]) + pm.P) for c in range(4)], []), dtype=np.uint64)
    return off, badt, z0, zero, big


def test_tile_schedule_vs_oracle(tile_emul, oracle):
    """Random tiles, the edge scalars, mixed bit lengths (lanes retire at different times), a ragged last tile, the
    identity point, and the invalid rows -- every output limb the oracle's, whichever way the gate sends a tile."""
    n = 6 * 64 + 23                                                                   # ragged: 23 lanes in the last tile
    P = V.base_multiples(oracle, n, V.SEED + 900)
    K = V.rand_scalars_np(n, V.SEED + 901, bits=252)
    rng = np.random.default_rng(V.SEED + 902)
    # tile 0: plain random 252-bit scalars (all valid).  tile 1: the edge rows and the raw patterns at or above 2^256
    edges = np.concatenate([np.array(edge_scalar_rows(), dtype=np.uint64), V.raw_scalar_edges()])[:64]
    K[64:64 + len(edges)] = edges
    # tile 2: mixed bit lengths, 1 .. 252 bits
    for j in range(64):
        bits = 1 + (j * 4) % 252
        v = (int.from_bytes(rng.bytes(32), "little") % (1 << bits)) | (1 << (bits - 1))
        K[128 + j] = pm.limbs(v)
    # tile 3: the identity point (and a sparse scalar, a dense one)
    P[192 + 5] = V.IDENT_ROW
    P[192 + 6] = V.IDENT_ROW
    K[192 + 6] = 0
    K[192 + 7] = pm.limbs(1 << 251)
    K[192 + 8] = pm.limbs((1 << 252) - 1)
    # tile 4: off the curve, inconsistent T, Z = 0 (each fails the gate); tile 5: the all-zero row and limbs >= p (both pass)
    off, badt, z0, zero, big = invalid_rows(oracle, V.SEED + 903)
    P[256 + 9], P[256 + 40], P[256 + 41] = off, badt, z0
    P[320 + 3], P[320 + 50] = zero, big
    # the ragged tile: one more invalid row among its 23 lanes
    P[384 + 11] = badt
    want = oracle.ed_scalar_mul(P, K)
    got, steps = run_tiles(tile_emul, P, K)
    assert np.array_equal(got, want)
    assert steps[:, 2].tolist() == [1, 1, 1, 1, 0, 1, 0]                              # tiles 4 and 6 took the fallback
    assert (steps[[4, 6], 1] == 0).all() and (steps[[0, 1, 2, 3, 5], 1] > 0).all()    # no doubling step there, some everywhere else
    # doubling steps switched off for every tile (ZC_SCHED=unified's schedule): the same limbs
    got_u, steps_u = run_tiles(tile_emul, P, K, allow_d=0)
    assert np.array_equal(got_u, want) and (steps_u[:, 1] == 0).all()


@pytest.mark.parametrize("kind", ["off_curve", "bad_t"])
def test_each_invalid_kind_takes_the_fallback(tile_emul, oracle, kind):
    """A tile whose only flaw is ONE off-curve row / ONE row with T Z != X Y must be seen to run without doubling steps
    (ptm_double_valid's G = (Y - X)(Y + X) is not the unified formula's D + C there), and still match the oracle."""
    n = 64
    P = V.base_multiples(oracle, n, V.SEED + 910)
    K = V.rand_scalars_np(n, V.SEED + 911, bits=252)
    off, badt = invalid_rows(oracle, V.SEED + 912)[:2]
    P[17] = off if kind == "off_curve" else badt
    got, steps = run_tiles(tile_emul, P, K)
    assert steps[0].tolist()[1:] == [0, 0]
    assert np.array_equal(got, oracle.ed_scalar_mul(P, K))
    # and the doubling body really differs on that row: with the gate overridden the tile cannot be trusted, so the kernel
    # never does this -- here only the all-valid twin of the tile is checked to take doubling steps
    P[17] = V.base_multiples(oracle, 1, V.SEED + 913)[0]
    got, steps = run_tiles(tile_emul, P, K)
    assert steps[0, 2] == 1 and steps[0, 1] > 100 and np.array_equal(got, oracle.ed_scalar_mul(P, K))


def test_step_counts_are_the_models(tile_emul, model, oracle):
    """Generic / doubling steps of every emulated tile == tools/sm_schedule_model.py's for the same scalars (depth 1), and
    the unified schedule's with doubling steps off: the dearest lane's bit length - 1 + popcount."""
    n = 5 * 64 + 9
    P = V.base_multiples(oracle, 8, V.SEED + 920)[np.arange(n) % 8]
    K = V.rand_scalars_np(n, V.SEED + 921, bits=252)
    order = np.argsort([-model.cost(pm.from_limbs(r)) for r in K], kind="stable")      # cost-sorted tiles, as the kernel sees them
    K = K[order]
    K[64:128] = V.rand_scalars_np(64, V.SEED + 922, bits=252)                          # one unsorted tile
    K[128:128 + 48] = np.concatenate([np.array(edge_scalar_rows(), dtype=np.uint64), V.raw_scalar_edges()])[:48]
    K[192:256, 2:] = 0                                                                 # short scalars (104 bits)
    _, steps = run_tiles(tile_emul, P, K)
    _, steps_u = run_tiles(tile_emul, P, K, allow_d=0)
    for t in range(len(steps)):
        vals = [pm.from_limbs(r) for r in K[64 * t:64 * t + 64]]
        g, d, _ = model.tile_steps(vals, depth=1)
        assert steps[t].tolist() == [g, d, 1], t
        assert steps_u[t].tolist() == [max(model.cost(v) for v in vals), 0, 0], t
        assert model.tile_steps(vals, depth=1, d_steps=False)[:2] == (steps_u[t, 0], 0)


def test_model_reproduces_the_design_figures(model):
    """Instruction-count ratios at stash depth 1 on the headline's input distribution: 0.907 (3S+5M) and 0.950 (4S+5M)."""
    tiles, mean_cost = model.sorted_tiles(model.bench_scalars(1 << 20, 0x5EED0003), 128)
    r = model.model(tiles, 1)
    assert abs(mean_cost - 376.0) < 0.05
    assert abs(r["ratio"]["3S+5M"] - 0.907) <= 0.002 and abs(r["ratio"]["4S+5M"] - 0.950) <= 0.002
    assert abs(r["generic"] - 188.9) < 0.1 and abs(r["doubling"] - 187.4) < 0.1 and abs(r["unified"] - 376.3) < 0.1


def test_tile_emul_under_asan_and_ubsan():
    """The same tiles with the host build under AddressSanitizer + UBSan (as tests/test_sanitizers.py does for emul.cpp)."""
    if os.environ.get("ZC_EMUL_SANITIZE"):
        pytest.skip("already inside the sanitizer run")
    rt = []
    for name in ("libasan.so", "libubsan.so"):
        path = subprocess.run(["gcc", "-print-file-name=" + name], capture_output=True, text=True).stdout.strip()
        if not (os.path.isabs(path) and os.path.exists(path)):
            pytest.skip("gcc's sanitizer runtimes are not installed")
        rt.append(path)
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "asan"], stdout=subprocess.DEVNULL)
    so = os.path.join(ROOT, "oracle", "libzc_ref_asan.so")
    preload = ":".join(rt + [x for x in [os.environ.get("LD_PRELOAD")] if x])
    env = dict(os.environ, LD_PRELOAD=preload, ZC_REF_SO=so, ZC_EMUL_SANITIZE="1",
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", os.path.abspath(__file__),
                          "-k", "vs_oracle or fallback or step_counts"], capture_output=True, text=True, cwd=ROOT, env=env, timeout=900)
    tail = (out.stdout + out.stderr)[-3000:]
    assert out.returncode == 0 and " passed" in out.stdout and "runtime error" not in tail and "AddressSanitizer" not in tail, tail
    assert os.path.exists(os.path.join(EMUL_DIR, "libzc_sm_tile_san.so")) and os.path.exists(os.path.join(EMUL_DIR, "libzc_sm_tile_san_checked.so"))
