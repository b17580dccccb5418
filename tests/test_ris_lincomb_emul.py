"""CPU tier: the per-lane core of zc_ris_lincomb (zc_curve.hip.h: ris_lincomb_decode / _table / _sum / _encode,
scalar_recode256, base_mul_onto) on waves of 64 real lanes.

tests/emul/ris_lincomb_emul.cpp drives the very functions k_ris_lincomb calls, through table_ptr, with the wave-level maxima
written as loops over the lanes and the basepoint comb built by the kernel's own column arithmetic -- so the decode into the
tables, the shared doubling chain, the comb additions on top of it and the accept mask are checked against the oracle's
composition of decompress, Mul<Scalar>, Add and compress before any GPU time is spent, in the plain, the bounds-asserting
and (ZC_EMUL_SANITIZE) the sanitizer build."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pymodel as pm
from tests import emul_build as EB
from tests import ris_lincomb_rows as RR
from tests import vectors as V
from tests.emul_build import EMUL_DIR, ROOT


@pytest.fixture(scope="module", params=["plain", "checked"])
def emul(request):
    checked = request.param == "checked"
    so = EB.library("ris_lincomb_emul.cpp", checked=checked, sanitize=bool(os.environ.get("ZC_EMUL_SANITIZE")))
    if so is None:
        pytest.skip("ROCm headers not present")
    return C.CDLL(so)


def run(lib, E, K, KB=None):
    E, K = np.ascontiguousarray(E, dtype=np.uint8), np.ascontiguousarray(K, dtype=np.uint64)
    KB = None if KB is None else np.ascontiguousarray(KB, dtype=np.uint64)
    n, t = E.shape[:2]
    out = np.full((n, 32), 0xA5, dtype=np.uint8)
    ok = np.full(n, 0xA5, dtype=np.uint8)
    tops = np.zeros((n + 63) // 64 * 2, dtype=np.int32)
    rc = lib.emul_ris_lincomb(E.ctypes.data_as(C.c_void_p), K.ctypes.data_as(C.c_void_p), C.c_size_t(t),
                              None if KB is None else KB.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                              ok.ctypes.data_as(C.c_void_p), C.c_size_t(n), tops.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return out, ok, tops.reshape(-1, 2)


@pytest.mark.parametrize("t,base", RR.CASES)
def test_ris_lincomb_core_vs_oracle(emul, oracle, t, base):
    """535 rows (a ragged last wave): the encodings of every planted scalar and point family, every family of undecodable
    encoding in every term position, the planted base scalars; all 32 bytes and the mask of every row are the oracle's."""
    n = 8 * 64 + 23
    E, K, KB, planted = RR.ris_lincomb_rows(oracle, n, t, V.SEED + 3000 + 10 * t + int(base), base)
    got, ok, tops = run(emul, E, K, KB)
    want = RR.oracle_ris_lincomb(oracle, E, K, KB)
    RR.assert_same_bytes((got, ok), want)
    assert planted == 5 * t and 0 < int((ok == 0).sum()) <= planted                      # random bytes decode now and then
    assert not got[ok == 0].any()
    assert tops[:, 0].max() == 65                                                        # a 260-bit pattern carries into the last digit
    assert (tops[:, 1].max() == 32) if base else (tops[:, 1] == -1).all()


def test_zero_waves_and_a_base_term_alone(emul, oracle):
    """A wave of all-zero scalars runs no window and no comb addition and yields 32 zero bytes with ok = 1; a wave whose
    only non-zero scalars are the base term's yields the encodings of kB * B (from the host-built comb alone); an
    undecodable row inside them is refused whatever its scalars."""
    t, n = 2, 3 * 64
    E = oracle.ris_compress(V.base_multiples(oracle, n * t, V.SEED + 3100)).reshape(n, t, 32).copy()
    K = V.rand_scalars_np(n * t, V.SEED + 3101, bits=252).reshape(n, t, 5)
    KB = V.rand_scalars_np(n, V.SEED + 3102, bits=252)
    K[:128] = 0
    KB[:64] = 0
    E[70, 1] = RR.le32(pm.P - 4)
    got, ok, tops = run(emul, E, K, KB)
    assert tops[0].tolist() == [-1, -1] and tops[1, 0] == -1 and tops[1, 1] >= 31 and tops[2, 0] >= 62
    assert not got[:64].any() and (ok[:64] == 1).all()
    RR.assert_same_bytes((got, ok), RR.oracle_ris_lincomb(oracle, E, K, KB))
    assert ok[70] == 0 and not got[70].any() and int((ok == 0).sum()) == 1
    keys = oracle.mt(oracle.ris_compress, oracle.mt(oracle.ed_scalar_mul, RR.basepoint_rows(64), KB[64:128]))
    rows = np.arange(64, 128) != 70
    assert np.array_equal(got[64:128][rows], keys[rows])


def test_base_digits_and_the_host_built_comb(emul, oracle):
    """digit i = byte i of (v + 0x80..80) - 128 is scalar_digits256's digit i, for random scalars, the edges and the raw
    patterns at or above 2^256; base_mul over the comb the emulation builds column by column is the oracle's k * B."""
    K = np.concatenate([V.rand_scalars_np(400, V.SEED + 3200, bits=252), V.rand_scalars_np(100, V.SEED + 3201, bits=260), V.raw_scalar_edges(),
                        np.array([[0] * 5, [1, 0, 0, 0, 0], [128, 0, 0, 0, 0], [127, 0, 0, 0, 0], pm.limbs(pm.L), pm.limbs(pm.L - 1), [(1 << 52) - 1] * 5,
                                  pm.limbs((1 << 252) - 1), pm.limbs(int("80" * 31, 16)), pm.limbs(int("7f" * 31, 16))], dtype=np.uint64)])
    n = len(K)
    rec, sto = np.zeros((n, 33), dtype=np.int8), np.zeros((n, 33), dtype=np.int8)
    tops = np.zeros((n, 2), dtype=np.int32)
    emul.emul_base_digits(K.ctypes.data_as(C.c_void_p), rec.ctypes.data_as(C.c_void_p), sto.ctypes.data_as(C.c_void_p),
                          tops.ctypes.data_as(C.c_void_p), C.c_size_t(n))
    assert np.array_equal(rec, sto) and np.array_equal(tops[:, 0], tops[:, 1])
    assert rec.min() == -128 and rec.max() == 127
    for i in range(400):
        assert sum(int(d) << (8 * j) for j, d in enumerate(rec[i])) == pm.from_limbs(K[i])
    got = np.zeros((n, 20), dtype=np.uint64)
    emul.emul_ed_mul_base(K.ctypes.data_as(C.c_void_p), got.ctypes.data_as(C.c_void_p), C.c_size_t(n))
    want = oracle.mt(oracle.ed_scalar_mul, RR.basepoint_rows(n), K)
    assert oracle.mt(oracle.ed_eq, got, want).all()
    assert np.array_equal(oracle.mt(oracle.ris_compress, got), oracle.mt(oracle.ris_compress, want))


def test_ris_lincomb_emul_under_asan_and_ubsan():
    """The same rows with the host build under AddressSanitizer + UBSan (as tests/test_lincomb_emul.py does)."""
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
                          "-k", "vs_oracle or zero_waves or base_digits"], capture_output=True, text=True, cwd=ROOT, env=env, timeout=1800)
    tail = (out.stdout + out.stderr)[-3000:]
    assert out.returncode == 0 and " passed" in out.stdout and "runtime error" not in tail and "AddressSanitizer" not in tail, tail
    assert os.path.exists(os.path.join(EMUL_DIR, "libzc_ris_lincomb_san.so")) and os.path.exists(os.path.join(EMUL_DIR, "libzc_ris_lincomb_san_checked.so"))
