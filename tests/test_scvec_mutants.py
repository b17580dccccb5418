"""CPU tier: defects planted in the scalar vector ops' device code must be caught by the rows of tests/scvec_rows.py.

The catalogue below is this feature's own (tests/mutants.py is left as it is).  Per entry the headers and the emulation source
are copied into a temporary directory, the one replacement is applied to the copied header, tests/emul/scvec_emul.cpp is built
from the copy with g++ -DZC_CHECK_BOUNDS (no sanitizer; a violated bound is counted, not fatal) and R.failures run on it: at
least one check must fail, and the families `killers` names must be among the failures (where `spared` names some, they must
pass).  Every planted defect stays inside the memory the emulation allocates (a shared b sits at the front of a zeroed
n x terms array there).  The unmutated copy passes, and every `old` text occurs exactly once in its header.  Nothing is written
inside the repository tree."""
import ctypes as C
import os

import pytest

from tests import emul_build as EB
from tests import scvec_rows as R
from tests.emul_build import CSRC

SCVEC, ARITH = "zc_scvec.hip.h", "zc_arith.hip.h"

MUTANTS = [
    # the carry pass comes after eight products: the values are still right (a column of 260-bit operands is below 8 * 2^58), the
    # bound the code is written to -- room for 9 * 2^58 before every product -- is not: the checked build reports it at the worst rows
    dict(name="carry_pass_one_product_late", header=SCVEC, old="if (pending == SCV_CARRY_EVERY) {", new="if (pending == SCV_CARRY_EVERY + 1) {", killers=["bounds"],
         spared=["sum", "dot", "dot_shared", "powers", "slice_sum"]),
    # the steps a launch walks are rounded down: the records of the last, ragged step are never read (and the last powers never written)
    dict(name="last_slice_tail_dropped", header=SCVEC, old="{ return (terms + parts - 1) / parts; }", new="{ return terms / parts; }", killers=["sum", "dot", "dot_shared", "powers"],
         cases=["sum [random n=1 terms=5]", "dot [random n=3 terms=1025]", "powers [bases n=1 terms=5]"], spared_cases=["sum [random n=1 terms=4]", "dot [random n=64 terms=8]"]),
    # a level of the tree with an odd number of partials loses its last one
    dict(name="trees_odd_partial_dropped", header=SCVEC, old="ZC_DI size_t scv_tree_half(size_t w) { return (w + 1) / 2; }", new="ZC_DI size_t scv_tree_half(size_t w) { return w / 2; }",
         killers=["sum", "dot"], spared=["powers", "slice_dot", "slice_sum", "bounds"], cases=["sum [random n=1 terms=32769]", "dot [worst n=1 terms=49152]"],
         spared_cases=["sum [random n=3 terms=32768]", "dot [random n=1 terms=49153]", "dot [random n=257 terms=513]"]),
    # every row reads b at its own row's offset although b is one row
    dict(name="shared_b_indexed_by_row", header=SCVEC, old="return (shared_b ? 0 : row * terms) + j;", new="return row * terms + j;", killers=["dot_shared"],
         spared=["sum", "dot", "powers", "slice_dot", "slice_sum", "bounds"], cases=["dot_shared [random n=63 terms=1]", "dot_shared [random n=3 terms=1025]"]),
    # the ladder squares once more: lanes step by x^(2 G)
    dict(name="x_to_the_G_off_by_one", header=SCVEC, old="for (u32 g = 1; g < G; g <<= 1) {", new="for (u32 g = 1; g <= G; g <<= 1) {", killers=["powers"],
         spared=["sum", "dot", "dot_shared", "slice_dot", "slice_sum", "bounds"], cases=["powers [bases n=64 terms=2]", "powers [bases n=1 terms=16385]"],
         spared_cases=["powers [bases n=63 terms=1]"]),
    # the first record of a row is x, not 1
    dict(name="first_power_taken_from_x", header=SCVEC, old="fe acc = fe_one_m<F>(); ", new="fe acc = l == 0 ? xm : fe_one_m<F>(); ", killers=["powers"],
         spared=["sum", "dot", "dot_shared", "slice_dot", "slice_sum", "bounds"], cases=["powers [bases n=63 terms=1]", "powers [bases n=65 terms=513]"]),
    # bits at and above 2^52 of a word reach the value
    dict(name="high_bits_of_a_word_not_masked", header=ARITH, old="u64 x = (l[idx] & M52) >> sh;", new="u64 x = l[idx] >> sh;", killers=["sum", "dot", "dot_shared", "powers", "slice_dot", "slice_sum"],
         cases=["sum [edges n=63 terms=7]", "dot [worst n=63 terms=1]"], spared_cases=["sum [random n=63 terms=7]", "dot [random n=65 terms=513]"]),
    # the nineteenth limb of a long slice is left out of the fold
    dict(name="nineteenth_limb_dropped", header=SCVEC, old="h.v[0] = (u32)(top >> 29);", new="h.v[0] = 0;", killers=["dot", "slice_dot"], spared=["sum", "powers", "slice_sum", "bounds"],
         cases=["slice_dot [worst m=5]", "dot [worst n=1 terms=1025]"], spared_cases=["dot [worst n=3 terms=1024]", "slice_dot [worst m=4]"]),
]
BY_NAME = {m["name"]: m for m in MUTANTS}


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    return EB.mutant_builds(tmp_path_factory, MUTANTS, "scvec_emul.cpp", flags=("-DZC_CHECK_BOUNDS",))


def test_catalogue_is_sound():
    EB.catalogue_is_sound(MUTANTS)
    assert 7 <= len(MUTANTS)
    scv = open(os.path.join(CSRC, SCVEC)).read()
    section = lambda a, b: scv[scv.index(a):scv.index(b)]
    assert BY_NAME["carry_pass_one_product_late"]["old"] in section("ZC_DI fe scv_slice_dot(", "ZC_DI fe scv_slice_sum(")
    assert BY_NAME["last_slice_tail_dropped"]["old"] in section("ZC_DI u32 scv_fold_steps(", "ZC_DI size_t scv_b_record(")
    assert BY_NAME["shared_b_indexed_by_row"]["old"] in section("ZC_DI size_t scv_b_record(", "ZC_DI fe scv_slice_dot(")
    for name in ("x_to_the_G_off_by_one", "first_power_taken_from_x"):
        assert BY_NAME[name]["old"] in section("ZC_DI void scv_pow_lane(", "// the kernels: hipcc only")
    assert BY_NAME["nineteenth_limb_dropped"]["old"] in section("ZC_DI fe scv_cols_fold(", "ZC_DI fe scv_pair(")
    arith = open(os.path.join(CSRC, ARITH)).read()
    assert BY_NAME["high_bits_of_a_word_not_masked"]["old"] in arith[arith.index("ZC_DI fe fe_from_limbs52("):arith.index("ZC_DI void fe_to_limbs52(")]
    # the kernels and the emulation go through the same functions
    kernels = scv[scv.index("// the kernels: hipcc only"):]
    for fn in ("scv_fold_steps(", "scv_b_record(", "scv_tree_half(", "scv_slice_dot(", "scv_slice_sum(", "scv_block_slice<", "scv_pow_lane(", "scv_pair("):
        assert fn in kernels, fn


def test_unmutated_copy_passes(built):
    assert R.failures(R.Emul(C.CDLL(built[None]))) == []


@pytest.mark.parametrize("name", [m["name"] for m in MUTANTS])
def test_planted_defect_is_killed(built, name):
    EB.assert_killed(BY_NAME[name], R.failures(R.Emul(C.CDLL(built[name]))))
