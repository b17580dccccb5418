"""CPU tier: fp_mul_d (zc_curve.hip.h), d x as x/m - x with d = 1/126297 - 1, built for the host by tests/emul/fe_muld_emul.cpp
in the plain and the bounds-asserting (-DZC_CHECK_BOUNDS) build.  tests/fe_muld_rows.py holds the inputs and the checks on
Python integers; the composed check runs the addition formulas that call the routine against the C oracle's ed_add on every
point class.  The sanitizer run is a stand-alone program (tests/emul/fe_muld_san.cpp) replaying a vector file as a child
process: nothing sanitized is loaded here."""
import ctypes as C
import struct

import numpy as np
import pytest

from oracle import pymodel as pm
from tests import emul_build as EB
from tests import fe_muld_rows as FM
from tests import point_classes as PC
from tests import vectors as V

FORMS = {0: "ptm_add", 1: "ptm_add ilp", 2: "pt_add", 3: "pt_add ilp", 4: "pt_add_plain", 5: "pt_add_plain ilp"}


@pytest.fixture(scope="module", params=["plain", "checked"])
def emul(request):
    so = EB.library("fe_muld_emul.cpp", checked=request.param == "checked")
    if so is None:
        pytest.skip("ROCm headers not present")
    return C.CDLL(so)


def test_model_on_integers(oracle):
    """The routine's steps on Python integers (FM.model asserts every one of them): y = (x + u p) / m, so y - x = d x."""
    names, x, want, res = FM.inputs(oracle)
    for i in list(range(len(names) - FM.N_RANDOM)) + list(range(len(names) - FM.N_RANDOM, len(names), 50)):
        u, carry, y = FM.model(x[i])
        assert (y - FM.value(x[i])) % pm.P == res[i] and y < 8.1 * pm.P and u < 8.1 * FM.MD, names[i]
    assert FM.value(x[0]) == 0 and FM.model(x[0])[2] == 0                                  # x = 0 gives y = 0, not 2^261


def test_every_input_gives_d_times_x(emul, oracle):
    assert FM.failures(emul, oracle) == []


def test_result_as_a_multiplier_operand(emul, oracle):
    """mont_mul(fp_mul_d(x), y) against an R-class partner at its largest limbs (the checked build asserts the column bound and
    the top-limb bound inside mont_mul) equals the two Montgomery products it replaces, and d x y R^-2 on integers."""
    names, x, _, res = FM.inputs(oracle)
    n = 4096
    x = x[:n].copy()
    y = np.roll(x, 1, axis=0).copy()
    y[0] = [FM.M29] * 8 + [FM.TOP_MAX]
    x[1] = FM.named_inputs(oracle)[7][1]                                                   # the largest input against the largest partner
    y[1] = y[0]
    got, want = np.zeros((n, 5), dtype=np.uint64), np.zeros((n, 5), dtype=np.uint64)
    emul.emul_fe_muld_times(C.c_void_p(x.ctypes.data), C.c_void_p(y.ctypes.data), C.c_void_p(got.ctypes.data), C.c_void_p(want.ctypes.data), C.c_size_t(n))
    assert np.array_equal(got, want)
    for i in range(0, n, 16):
        assert pm.from_limbs([int(w) for w in got[i]]) == pm.D * FM.value(x[i]) * FM.value(y[i]) * FM.RINV * FM.RINV % pm.P


@pytest.fixture(scope="module")
def pairs(oracle):
    """(p, q, oracle ed_add): every row of every point class against its neighbour, itself, its class's next row and the identity."""
    rows, names = PC.interleave(PC.classes(oracle, 64, FM.SEED))
    p = np.concatenate([rows, rows, rows, rows, PC.ident_rows(len(rows))])
    q = np.concatenate([np.roll(rows, 1, axis=0), rows, np.roll(rows, len(PC.CLASS_NAMES) + 1, axis=0), PC.ident_rows(len(rows)), rows])
    p, q = np.ascontiguousarray(p), np.ascontiguousarray(q)
    return p, q, oracle.mt(oracle.ed_add, p, q)


@pytest.mark.parametrize("form", sorted(FORMS), ids=[FORMS[f].replace(" ", "-") for f in sorted(FORMS)])
def test_addition_formulas_match_the_oracle(emul, pairs, form):
    p, q, want = pairs
    out = np.zeros_like(p)
    emul.emul_muld_ed_add(C.c_void_p(p.ctypes.data), C.c_void_p(q.ctypes.data), C.c_void_p(out.ctypes.data), C.c_size_t(len(p)), form)
    assert np.array_equal(out, want), FORMS[form]


def test_stand_alone_program_under_asan_and_ubsan(tmp_path, oracle, pairs):
    """tests/emul/fe_muld_san.cpp with -fsanitize=address,undefined -fno-sanitize-recover=all and the bounds assertions on the
    named inputs, 4 000 random ones and the point pairs in every form; its exit status is the verdict."""
    exe = EB.sanitizer_program("fe_muld_san.cpp", tmp_path, checked=True)
    names, x, want, _ = FM.inputs(oracle)
    n = len(names) - FM.N_RANDOM + 4000
    blob = struct.pack("<QQ", 1, n) + np.ascontiguousarray(x[:n]).tobytes() + np.ascontiguousarray(want[:n]).tobytes()
    p, q, sums = pairs
    for form in sorted(FORMS):
        blob += struct.pack("<QQ", 2 + form, 512) + p[-700:-188].tobytes() + q[-700:-188].tobytes() + sums[-700:-188].tobytes()
    blob += struct.pack("<QQ", 0, 0)
    EB.assert_clean(EB.run_vectors(exe, blob, tmp_path, "vectors.bin"), "rows match")
    # the verdict is a real one: one expected limb changed and the program says so
    bad = bytearray(blob)
    bad[16 + 36 * n + 40 * 3 + 8] ^= 1                                                     # limb 1 of row 3 of the first record's expected values
    EB.assert_caught(EB.run_vectors(exe, bad, tmp_path, "wrong.bin"), "row 3 word 1")
