"""CPU tier: defects planted in the generator sets' device code must be caught by the rows of tests/gens_rows.py.

The catalogue below is this feature's own (tests/mutants.py is left as it is).  Per entry the headers and the emulation source
are copied into a temporary directory, the one replacement is applied to the copied header, tests/emul/gens_emul.cpp is built
from the copy with g++ (no sanitizer, no bounds assertions) and GR.failures run on it: at least one check must fail, and the
families `killers` names must be among the failures (where `spared` names some, they must pass).  Every planted defect stays
inside the tables the emulation allocates.  The unmutated copy passes, and every `old` text occurs exactly once in its header.
Nothing is written inside the repository tree."""
import ctypes as C
import os

import pytest

from tests import emul_build as EB
from tests import gens_rows as GR
from tests.emul_build import CSRC

GENS, CURVE = "zc_gens.hip.h", "zc_curve.hip.h"
ROWS = ["ed", "wire"]

MUTANTS = [
    # term j reads the table of term j - 1: one generator is untouched, every longer list is wrong
    dict(name="term_table_of_the_previous_term", header=GENS, old="tables + (size_t)j * GENS_TABLE_WORDS, rw, stride, top);",
         new="tables + (size_t)(j ? j - 1 : 0) * GENS_TABLE_WORDS, rw, stride, top);", killers=ROWS, cases=["ed [count=2]", "wire [count=8]"], spared_cases=["ed [count=1]"]),
    # tables 32 windows apart: window 0 of table j + 1 lies over window 32 of table j, which only scalars from 2^256 up read
    dict(name="table_stride_of_32_windows", header=GENS, old="GENS_TABLE_WORDS = (size_t)ZC_BASE_WINDOWS * ZC_BASE_ENTRIES * 32;",
         new="GENS_TABLE_WORDS = (size_t)(ZC_BASE_WINDOWS - 1) * ZC_BASE_ENTRIES * 32;", killers=ROWS, cases=["ed [count=3]", "wire [count=2]"]),
    dict(name="window_32_not_built", header=CURVE, old="for (int w = 0; w < ZC_BASE_WINDOWS; w++) {", new="for (int w = 0; w < ZC_BASE_WINDOWS - 1; w++) {",
         killers=ROWS + ["basepoint"], cases=["ed [count=1]"]),
    dict(name="t_taken_from_the_input", header=GENS, old="G.T = fp_mul(G.X, G.Y);", new="G.T = fe_load_mont<FP>(p + 15);", killers=ROWS, cases=["ed [count=1]", "wire [count=8]"],
         spared=["basepoint", "refusals"]),
    dict(name="x_not_normalised", header=GENS, old="G.X = fp_mul(P.X, zi);", new="G.X = P.X;", killers=ROWS, cases=["wire [count=1]"], spared=["basepoint", "refusals"]),
    dict(name="z_zero_accepted", header=GENS, old="const bool ok = ed_is_valid(P) && !fp_is_zero(P.Z);", new="const bool ok = ed_is_valid(P);", killers=["refusals"],
         cases=["refusals [Z = 0]", "refusals [Z = 0 last]"], spared=ROWS + ["basepoint"]),
    dict(name="scalars_in_reverse_order", header=GENS, old="load_scalar(l, k + 5 * j);", new="load_scalar(l, k + 5 * (count - 1 - j));", killers=ROWS, cases=["ed [count=2]"],
         spared_cases=["ed [count=1]"]),
]
BY_NAME = {m["name"]: m for m in MUTANTS}


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    return EB.mutant_builds(tmp_path_factory, MUTANTS, "gens_emul.cpp")


def test_catalogue_is_sound():
    EB.catalogue_is_sound(MUTANTS)
    assert 4 <= len(MUTANTS)
    gens = open(os.path.join(CSRC, GENS)).read()
    curve = open(os.path.join(CSRC, CURVE)).read()
    # the window loop that is cut short is the generalised column builder's
    body = curve[curve.index("ZC_DI void comb_table_column("):curve.index("ZC_DI void base_table_column(")]
    assert BY_NAME["window_32_not_built"]["old"] in body
    for name in ("term_table_of_the_previous_term", "scalars_in_reverse_order"):
        body = gens[gens.index("ZC_DI pt gens_row_sum("):gens.index("#if defined(__HIPCC__)")]
        assert BY_NAME[name]["old"] in body


def test_unmutated_copy_passes(built, oracle):
    assert GR.failures(C.CDLL(built[None]), oracle) == []


@pytest.mark.parametrize("name", [m["name"] for m in MUTANTS])
def test_planted_defect_is_killed(built, oracle, name):
    EB.assert_killed(BY_NAME[name], GR.failures(C.CDLL(built[name]), oracle))
