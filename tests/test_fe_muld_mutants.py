"""CPU tier: defects planted in fp_mul_d must be caught by the vectors of tests/fe_muld_rows.py.

The catalogue below is this routine's own (tests/mutants.py is left as it is).  Per entry the headers and the emulation sources
are copied into a temporary directory, the one replacement is applied to the copied header, tests/emul/fe_muld_emul.cpp is
built from the copy with g++ (no sanitizer, no bounds assertions) and FM.failures run on it: at least one input must fail,
and where `killers` names inputs, those must be among the failures.  The unmutated copy passes, and every `old` text
occurs exactly once in its header.  Nothing is written inside the repository tree."""
import ctypes as C

import pytest

from tests import emul_build as EB
from tests import fe_muld_rows as FM

CURVE, CONSTANTS = "zc_curve.hip.h", "zc_constants.hip.h"

MUTANTS = [
    # z' = x + u p without the offset: the complement is then z'/m - 1 on every input, and 2^261 - 1 where z' = 0
    dict(name="offset_m_dropped", header=CURVE, old="u32 carry = F::MD;", new="u32 carry = 0;", killers=["zero"]),
    dict(name="k_3_wrong", header=CONSTANTS, old="MD_K[9] = {16607, 18298, 3605, 79513,", new="MD_K[9] = {16607, 18298, 3605, 79514,", killers=["limb 3 alone"]),
    dict(name="nminv_wrong_sign", header=CONSTANTS, old="MD_NMINV = 0x03ea7517u", new="MD_NMINV = 0x1c158ae9u", killers=["one"]),
    dict(name="complement_mask_30_bits", header=CURVE, old="(v ^ M29) +", new="(v ^ 0x3fffffffu) +", killers=["zero", "one"]),
    dict(name="barrett_shift_17", header=CURVE, old="(u64)(u32)(s >> 18) *", new="(u64)(u32)(s >> 17) *", killers=["p - 1"]),
    dict(name="barrett_shift_19", header=CURVE, old="(u64)(u32)(s >> 18) *", new="(u64)(u32)(s >> 19) *", killers=["p - 1"]),
    dict(name="minus_x_dropped", header=CURVE, old="(v ^ M29) + (F::BIAS[i] - x.v[i]);", new="(v ^ M29) + F::BIAS[i];", killers=["one", "p - 1"]),
]
BY_NAME = {m["name"]: m for m in MUTANTS}
assert (0x03ea7517 + 0x1c158ae9) == 1 << 29


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    return EB.mutant_builds(tmp_path_factory, MUTANTS, "fe_muld_emul.cpp")


def test_catalogue_is_sound():
    EB.catalogue_is_sound(MUTANTS)


def test_unmutated_copy_passes(built, oracle):
    assert FM.failures(C.CDLL(built[None]), oracle) == []


@pytest.mark.parametrize("name", [m["name"] for m in MUTANTS])
def test_planted_defect_is_killed(built, oracle, name):
    EB.assert_killed(BY_NAME[name], FM.failures(C.CDLL(built[name]), oracle))
