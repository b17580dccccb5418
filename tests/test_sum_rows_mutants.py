"""CPU tier: defects planted in the point sums' device code and host plan must be caught by the rows of tests/sum_rows.py.

The catalogue below is this feature's own (tests/mutants.py is left as it is).  Per entry the headers and the emulation source
are copied into a temporary directory, the one replacement is applied to the copied header, tests/emul/sum_rows_emul.cpp is
built from the copy with g++ (no sanitizer, no bounds assertions) and SR.failures run on it: at least one check must fail, the
families `killers` names must be among the failures, the families `spared` names must pass, and so must every `spared_cases`
label.  The unmutated copy passes, and every `old` text occurs exactly once in its header.  Nothing is written inside the
repository tree.

The fold started from the identity (identity + P_0 + ...) is the same group element in other coordinates: it fails the limb
checks -- of every term count from 1 up, the one-term row that must be its point among them -- and nothing else; it spares the
families "ed_eq" (group equality and compressed bytes) and "wire" (an encoding depends on the group element only), in the
Edwards fold and in the wire fold alike.  Only limb-for-limb comparison against the model tells it apart."""
import ctypes as C
import os

import pytest

from tests import emul_build as EB
from tests import sum_rows as SR
from tests.emul_build import CSRC

SUM, PLAN = "zc_sum.hip.h", "zc_sum_plan.h"
ALL = ["ed", "ed_eq", "wire"]

MUTANTS = [
    # stride P - 1 between the points of a slice: with one part every step reads point 0 again
    dict(name="slice_stride_of_parts_minus_one", header=SUM, old="const size_t j = s + k * parts;", new="const size_t j = s + k * (parts - 1);", killers=["ed", "ed_eq"],
         spared=["wire"], cases=["ed [terms=2]", "ed [terms=33]", "ed [terms=8197]"], spared_cases=["ed [terms=1]"]),
    dict(name="wire_slice_stride_of_parts_minus_one", header=SUM, old="left--, j += parts) {", new="left--, j += parts - 1) {", killers=["wire"],
         spared=["ed", "ed_eq"], cases=["wire [terms=3]", "wire [terms=4096]"], spared_cases=["wire [terms=1]"]),
    # the last, shorter step of uneven slices dropped (sum_fold_steps, which the kernels and the emulation call): only term
    # counts that are no multiple of their parts notice
    dict(name="last_shorter_step_dropped", header=SUM, old="{ return (terms + parts - 1) / parts; }", new="{ return terms / parts; }", killers=ALL,
         cases=["ed [terms=33]", "ed [terms=47]", "wire [terms=8197]"], spared_cases=["ed [terms=8]", "ed [terms=4096]", "wire [terms=4096]"]),
    # a tree level that pairs s with s + 1 at odd s: shows from 4 parts on
    dict(name="tree_pairs_s_with_s_plus_1_at_odd_s", header=SUM, old="sum_partial_get(q, 2 * s, es, ws, oa);", new="sum_partial_get(q, 2 * s + (s & 1), es, ws, oa);", killers=ALL,
         cases=["ed [terms=100]", "ed [terms=4096]", "wire [terms=8197]"], spared_cases=["ed [terms=33]", "ed [terms=47]", "wire [terms=47]"]),
    dict(name="tree_stopped_one_level_early", header=SUM, old="{ return width > 1; }", new="{ return width > 2; }", killers=ALL,
         cases=["ed [terms=33]", "ed [terms=100]", "wire [terms=4096]"], spared_cases=["ed [terms=8]", "wire [terms=8]"]),
    dict(name="accept_bit_ored_in_the_fold", header=SUM, old="okw = okw & (dec ? 1u : 0u);", new="okw = okw | (dec ? 1u : 0u);", killers=["wire"], spared=["ed", "ed_eq"],
         cases=["wire [terms=1]", "wire [terms=3]", "wire [terms=8197]"], spared_cases=["wire [terms=0]"]),
    dict(name="accept_bit_ored_in_the_tree", header=SUM, old="ok = oa && ob;", new="ok = oa || ob;", killers=["wire"], spared=["ed", "ed_eq"],
         cases=["wire [terms=33]", "wire [terms=4096]"], spared_cases=["wire [terms=8]"]),
    dict(name="fold_started_from_the_identity", header=SUM, old="if (have) acc = k == 0 ? ptm_from_pt(P) : ptm_add(acc, ptm_from_pt(P));",
         new="if (have) acc = ptm_add(acc, ptm_from_pt(P));", killers=["ed"], spared=["ed_eq", "wire"], cases=["ed [terms=1]", "ed [terms=2]", "ed [terms=4096]"],
         spared_cases=["ed [terms=0]"]),
    dict(name="wire_fold_started_from_the_identity", header=SUM, old="acc = ZC_SUM_UNIFORM(fresh) ? m : ptm_add(acc, m);", new="acc = ptm_add(acc, m);", killers=[], survives=True),
]
BY_NAME = {m["name"]: m for m in MUTANTS}


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    return EB.mutant_builds(tmp_path_factory, MUTANTS, "sum_rows_emul.cpp")


def test_catalogue_is_sound():
    EB.catalogue_is_sound(MUTANTS)
    assert 6 <= len(MUTANTS)
    text = open(os.path.join(CSRC, SUM)).read()
    device = text[:text.index("#if defined(__HIPCC__)")]                                # what the emulation builds: the functions the kernels call
    for m in MUTANTS:
        if m["header"] == SUM:
            assert m["old"] in device, m["name"]
    kernels = text[text.index("#if defined(__HIPCC__)"):]
    for fn in ("sum_slice_fold(", "sum_wire_slice_fold(", "sum_tree_pair(", "sum_tree_more("):
        assert fn in kernels, fn                                                        # the kernels run the mutated functions, not copies
    assert "const u32 steps = sum_fold_steps(terms, parts);" in kernels                # the step count that is cut short is the kernels' own


def test_unmutated_copy_passes(built, oracle):
    assert SR.failures(C.CDLL(built[None]), oracle) == []


@pytest.mark.parametrize("name", [m["name"] for m in MUTANTS])
def test_planted_defect_is_killed(built, oracle, name):
    m = BY_NAME[name]
    failed = SR.failures(C.CDLL(built[name]), oracle)
    if m.get("survives"):
        assert failed == [], (name, failed)                                             # the same group element: no byte of the wire form can tell
        return
    EB.assert_killed(m, failed)
