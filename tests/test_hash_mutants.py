"""CPU tier: defects planted in the SHA-512 rows must be caught by the vectors of tests/hash_rows.py.

The catalogue below is this header's own (tests/mutants.py is left as it is).  Per entry the headers and the emulation source
are copied into a temporary directory, the one replacement is applied to the copied zc_hash.hip.h, tests/emul/hash_emul.cpp is
built from the copy with g++ (no sanitizer, no bounds assertions) and HR.failures run on it: at least one vector must fail, and
where `killers` names families of vectors, those must be among the failures (and where `spared` names some, they must pass: a
defect of one reader form leaves the other alone).  The unmutated copy passes, and every `old` text occurs exactly once in the
header.  Nothing is written inside the repository tree."""
import ctypes as C
import os

import pytest

from tests import emul_build as EB
from tests import hash_rows as HR
from tests.emul_build import CSRC

HASH = "zc_hash.hip.h"
CH_MAJ = ("ZC_DI u64 sha512_ch(u64 e, u64 f, u64 g) { return g ^ (e & (f ^ g)); }\n"
          "ZC_DI u64 sha512_maj(u64 a, u64 b, u64 c) { return (a & b) | (c & (a | b)); }")
MAJ_CH = ("ZC_DI u64 sha512_maj(u64 e, u64 f, u64 g) { return g ^ (e & (f ^ g)); }\n"
          "ZC_DI u64 sha512_ch(u64 a, u64 b, u64 c) { return (a & b) | (c & (a | b)); }")
DIGEST = ["stream", "digest word", "digest bytes"]

MUTANTS = [
    dict(name="Sigma0_rotation_29", old="rotr64<28>(x)", new="rotr64<29>(x)", killers=DIGEST),
    dict(name="Sigma1_rotation_15", old="rotr64<14>(x)", new="rotr64<15>(x)", killers=DIGEST),
    dict(name="sigma0_rotation_2", old="rotr64<1>(x)", new="rotr64<2>(x)", killers=DIGEST),
    dict(name="sigma1_rotation_20", old="rotr64<19>(x)", new="rotr64<20>(x)", killers=DIGEST),
    dict(name="ch_and_maj_swapped", old=CH_MAJ, new=MAJ_CH, killers=DIGEST),
    dict(name="round_constant_low_bit", old="0x5fcb6fab3ad6faecull", new="0x5fcb6fab3ad6faedull", killers=["tables"] + DIGEST),
    dict(name="length_in_bytes", old="x = (u64)m.total * 8;", new="x = (u64)m.total;", killers=["digest word", "digest bytes"], spared=["stream"]),
    dict(name="marker_one_byte_late_byte_form", old="p == m.total ? 0x80u", new="p == m.total + 1 ? 0x80u", killers=["digest bytes"], spared=["stream", "digest word"]),
    dict(name="marker_one_byte_late_word_form", old="return 0x8000000000000000ull;", new="return 0x0080000000000000ull;", killers=["digest word"],
         spared=["stream", "digest bytes"]),
    dict(name="padding_decision_ge_111", old="(total & 127) > 111", new="(total & 127) >= 111", killers=["digest bytes"], cases=["prefix=0 parts=111", "prefix=0 parts=239"]),
    dict(name="byte_swap_dropped_in_the_word_form", old="return __builtin_bswap64(hash_load8_aligned(", new="return (hash_load8_aligned(", killers=["digest word"],
         spared=["stream", "digest bytes"]),
    dict(name="digest_reversed_before_the_reduction", old="d[k] = __builtin_bswap64(state[k]);", new="d[7 - k] = state[k];", killers=["scalar", "scalar edges"],
         spared=DIGEST),
]
BY_NAME = {m["name"]: m for m in MUTANTS}


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    return EB.mutant_builds(tmp_path_factory, MUTANTS, "hash_emul.cpp", headers=HASH)


def test_catalogue_is_sound():
    EB.catalogue_is_sound(MUTANTS, headers=HASH)
    text = open(os.path.join(CSRC, HASH)).read()
    # the four rotation entries sit in the four functions they name, the constant is the table's 79th
    for fn, old in (("sha512_Sigma0", "rotr64<28>(x)"), ("sha512_Sigma1", "rotr64<14>(x)"), ("sha512_sigma0", "rotr64<1>(x)"), ("sha512_sigma1", "rotr64<19>(x)")):
        line = next(l for l in text.split("\n") if l.startswith("ZC_DI u64 %s(" % fn))
        assert old in line, fn
    assert HR.round_constants()[78] == 0x5fcb6fab3ad6faec


def test_unmutated_copy_passes(built, oracle):
    assert HR.failures(C.CDLL(built[None]), oracle) == []


@pytest.mark.parametrize("name", [m["name"] for m in MUTANTS])
def test_planted_defect_is_killed(built, oracle, name):
    m = BY_NAME[name]
    failed = HR.failures(C.CDLL(built[name]), oracle)
    EB.assert_killed({k: v for k, v in m.items() if k != "cases"}, failed)
    for case in m.get("cases", []):                                                      # here a case names the vector, whichever family fails on it
        assert any(f.endswith("[%s]" % case) for f in failed), (name, case)
