"""CPU tier: the per-lane core of zc_ed_lincomb (zc_curve.hip.h: scalar_recode16, lincomb_fast) on waves of 64 real lanes.

tests/emul/lincomb_emul.cpp drives the very functions k_ed_lincomb calls, through table_ptr, with the wave-level maximum of
the top window written as a loop over the lanes -- so the shared doubling chain, the per-term tables and the on-the-fly
digits are checked against the oracle's composition of Mul<Scalar> and Add before any GPU time is spent, in the plain, the
bounds-asserting and (ZC_EMUL_SANITIZE) the sanitizer build."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pymodel as pm
from tests import emul_build as EB
from tests import lincomb_rows as R
from tests import vectors as V
from tests.emul_build import EMUL_DIR, ROOT

TERMS = [1, 2, 3, 4, 5, 8]


@pytest.fixture(scope="module", params=["plain", "checked"])
def emul(request):
    checked = request.param == "checked"
    so = EB.library("lincomb_emul.cpp", checked=checked, sanitize=bool(os.environ.get("ZC_EMUL_SANITIZE")))
    if so is None:
        pytest.skip("ROCm headers not present")
    return C.CDLL(so)


def run_lincomb(lib, P, K):
    P, K = np.ascontiguousarray(P, dtype=np.uint64), np.ascontiguousarray(K, dtype=np.uint64)
    n, t = P.shape[:2]
    out = np.zeros((n, 20), dtype=np.uint64)
    tops = np.zeros((n + 63) // 64, dtype=np.int32)
    strict = C.c_int(0)
    rc = lib.emul_ed_lincomb(P.ctypes.data_as(C.c_void_p), K.ctypes.data_as(C.c_void_p), C.c_size_t(t), out.ctypes.data_as(C.c_void_p),
                             C.c_size_t(n), tops.ctypes.data_as(C.c_void_p), C.byref(strict))
    assert rc == 0
    return out, tops, strict.value


@pytest.mark.parametrize("t", TERMS)
def test_lincomb_core_vs_oracle(emul, oracle, t):
    """535 rows (a ragged last wave) with every planted family; every row is the oracle's ((k0 P0 + k1 P1) + ...)."""
    n = 8 * 64 + 23
    P, K, where = R.lincomb_rows(oracle, n, t, V.SEED + 1000 + 10 * t)
    assert len(where) >= 60 and len(set(p // 64 for p in where)) >= 7
    got, tops, strict = run_lincomb(emul, P, K)
    R.assert_same_points(oracle, got, R.oracle_lincomb(oracle, P, K))
    assert tops.max() == 65                                                           # a 260-bit pattern carries into the last digit
    # One of the three points ed_coset4 adds to the identity, (1, 0), is NOT on the curve (the reference's FOUR_COSET_GROUP
    # holds it as it is): no windowed schedule reproduces the unified formula there, the rows that hold it take the
    # reference's own sequence -- those rows and no others.
    on_curve = oracle.ed_is_valid(P.reshape(-1, 20)).reshape(n, t).all(axis=1)
    assert strict == int((~on_curve).sum()) == 2
    if t == 1:
        fast = np.zeros_like(got)
        p1, k1 = np.ascontiguousarray(P[:, 0]), np.ascontiguousarray(K[:, 0])
        emul.emul_ed_scalar_mul_fast(p1.ctypes.data_as(C.c_void_p), k1.ctypes.data_as(C.c_void_p), fast.ctypes.data_as(C.c_void_p), C.c_size_t(n))
        assert oracle.ed_eq(got[on_curve], fast[on_curve]).all()                      # the windowed multiplication has no such gate


def test_short_waves_stop_at_their_own_top(emul, oracle):
    """A wave of short scalars runs from its own top window (the maximum over its rows' terms), an all-zero wave runs no
    window at all and yields identities; the neighbouring full-length wave is not affected."""
    t, n = 3, 3 * 64
    P = V.base_multiples(oracle, n * t, V.SEED + 1100).reshape(n, t, 20)
    K = V.rand_scalars_np(n * t, V.SEED + 1101, bits=252).reshape(n, t, 5)
    K[:64] = 0
    K[64:128, :, 1:] = 0                                                               # 52-bit scalars
    K[64:128, :, 0] |= np.uint64(1 << 51)
    got, tops, strict = run_lincomb(emul, P, K)
    assert strict == 0 and tops[0] == -1 and tops[1] == 13 and tops[2] >= 62
    assert oracle.ed_eq(got[:64], np.tile(np.array([V.IDENT_ROW], dtype=np.uint64), (64, 1))).all()
    R.assert_same_points(oracle, got, R.oracle_lincomb(oracle, P, K))


def test_recoded_digits_are_the_stored_digits(emul):
    """digit i = nibble i of (v + 0x88..8) - 8 is scalar_digits16's digit i, for random scalars, the edges and the raw
    patterns at or above 2^256; the value of the digit string is the effective scalar."""
    K = np.concatenate([V.rand_scalars_np(400, V.SEED + 1200, bits=252), V.rand_scalars_np(100, V.SEED + 1201, bits=260), V.raw_scalar_edges(),
                        np.array([[0] * 5, [1, 0, 0, 0, 0], [8, 0, 0, 0, 0], [7, 0, 0, 0, 0], pm.limbs(pm.L), pm.limbs(pm.L - 1), [(1 << 52) - 1] * 5,
                                  pm.limbs((1 << 252) - 1), pm.limbs(int("8" * 63, 16)), pm.limbs(int("7" * 63, 16))], dtype=np.uint64)])
    n = len(K)
    rec, sto = np.zeros((n, 66), dtype=np.int8), np.zeros((n, 66), dtype=np.int8)
    tops = np.zeros((n, 2), dtype=np.int32)
    emul.emul_lincomb_digits(K.ctypes.data_as(C.c_void_p), rec.ctypes.data_as(C.c_void_p), sto.ctypes.data_as(C.c_void_p),
                             tops.ctypes.data_as(C.c_void_p), C.c_size_t(n))
    assert np.array_equal(rec, sto) and np.array_equal(tops[:, 0], tops[:, 1])
    assert rec.min() >= -8 and rec.max() <= 7
    for i in range(400, 400 + 100):                                                    # 260-bit values below 2^256 ... 2^260: all bits count unless the loop stops early
        v = sum(int(d) << (4 * j) for j, d in enumerate(rec[i]))
        raw = pm.from_limbs(K[i])
        assert v == raw or (raw >> 256 and v == raw % (1 << 256))


def test_lincomb_emul_under_asan_and_ubsan():
    """The same rows with the host build under AddressSanitizer + UBSan (as tests/test_sm_schedule_emul.py does)."""
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
                          "-k", "vs_oracle or short_waves or recoded"], capture_output=True, text=True, cwd=ROOT, env=env, timeout=1800)
    tail = (out.stdout + out.stderr)[-3000:]
    assert out.returncode == 0 and " passed" in out.stdout and "runtime error" not in tail and "AddressSanitizer" not in tail, tail
    assert os.path.exists(os.path.join(EMUL_DIR, "libzc_lincomb_san.so")) and os.path.exists(os.path.join(EMUL_DIR, "libzc_lincomb_san_checked.so"))
