"""CPU tier: defects planted in the bounded discrete logs' device code and host plan must be caught by the rows of
tests/dlog_rows.py.

The catalogue below is this feature's own (tests/mutants.py is left as it is).  Per entry the headers and the emulation source
are copied into a temporary directory, the one replacement is applied to the copied header, tests/emul/dlog_emul.cpp is built
from the copy with g++ (no sanitizer, no bounds assertions) and DR.failures run on it: at least one check must fail, and the
families `killers` names must be among the failures (where `spared` names some, they must pass).  Every planted defect stays
inside the memory the emulation allocates.  The unmutated copy passes, and every `old` text occurs exactly once in its header.
Nothing is written inside the repository tree."""
import ctypes as C
import os

import pytest

from tests import dlog_rows as DR
from tests import emul_build as EB
from tests.emul_build import CSRC

DLOG, PLAN = "zc_dlog.hip.h", "zc_dlog_plan.h"

MUTANTS = [
    # a match in the last giant step at or above the bound is reported
    dict(name="bound_test_dropped", header=DLOG, old="if (j >= 0 && m < bound) {", new="if (j >= 0) {", killers=["ed", "cut", "wire"], spared=["table", "record", "refusals"],
         cases=["ed [B t=4 coset4=0]", "wire [multiple t=6 coset4=1]"]),
    # the builder leaves bit 255 clear: the table is not the fingerprint the header promises
    dict(name="parity_bit_left_out_of_the_record", header=DLOG, old="        w[3] |= dlog_chunk_x_parity(I, stage, stride, i) << 63;\n", new="", killers=["table"],
         cases=["table [B t=4 coset4=0]", "table [mixed t=6 coset4=1]"]),
    # the last step of every chunk is never looked up
    dict(name="last_step_of_a_chunk_skipped", header=DLOG, old="if (live && !found) {", new="if (live && !found && i != DLOG_CHUNK - 1) {", killers=["ed", "cut", "wire"],
         spared=["table", "record"], cases=["ed [multiple t=4 coset4=1]"]),
    # launch k starts from the offset of launch k - 1: rows beyond 1024 giant steps are lost; the cut search works its offsets out itself
    dict(name="offset_of_the_previous_launch", header=PLAN, old="(DLOG_SETUP_W + (size_t)k); }", new="(DLOG_SETUP_W + (size_t)(k ? k - 1 : 0)); }", killers=["ed", "wire"],
         spared=["table", "record", "cut", "refusals"], cases=["ed [mixed t=6 coset4=0]"]),
    # a row is not multiplied by four for a table of 4 G
    dict(name="coset4_doublings_dropped", header=DLOG, old="    if (coset4) {\n", new="    if (false && coset4) {\n", killers=["ed", "cut", "wire"], spared=["table", "record", "refusals"],
         cases=["ed [B t=4 coset4=1]", "wire [B t=4 coset4=1]"], spared_cases=["ed [B t=4 coset4=0]", "ed [mixed t=6 coset4=0]"]),
    # two slots are read whatever they hold: a record that linear probing moved further is never found
    dict(name="fixed_number_of_slots_read", header=DLOG,
         old="    for (size_t s = dlog_home(w[0], T.t);; s = dlog_next(s, T.t)) {\n        const u64 slot = T.slots[s];\n        if (slot == DLOG_EMPTY) break;\n",
         new="    size_t s = dlog_home(w[0], T.t);\n    for (int tries = 0; tries < 2; tries++, s = dlog_next(s, T.t)) {\n        const u64 slot = T.slots[s];\n        if (slot == DLOG_EMPTY) continue;\n",
         killers=["ed"], spared=["table", "record", "refusals"]),
    # a matching y is taken for +j G without asking the neighbouring giant step: -j G gives a wrong m
    dict(name="sign_not_decided", header=DLOG, old="else if (hit > 0 && dlog_y_is(T, above, size - (size_t)hit)) j = hit;", new="else if (hit > 0) j = hit;", killers=["ed", "cut"],
         spared=["table", "record"], cases=["ed [B t=4 coset4=0]"]),
    # the chunk's last step is judged like the others, by a y that is not there
    dict(name="last_step_judged_without_its_neighbour", header=DLOG, old="else if (hit > 0 && i == DLOG_CHUNK - 1) waiting = hit;\n", new="", killers=["ed"], spared=["table", "record"]),
]
BY_NAME = {m["name"]: m for m in MUTANTS}


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    return EB.mutant_builds(tmp_path_factory, MUTANTS, "dlog_emul.cpp")


def test_catalogue_is_sound(oracle):
    EB.catalogue_is_sound(MUTANTS)
    assert 6 <= len(MUTANTS)
    dlog = open(os.path.join(CSRC, DLOG)).read()
    search = dlog[dlog.index("ZC_DI bool dlog_search("):dlog.index("ZC_DI bool dlog_load_ed(")]
    for name in ("bound_test_dropped", "last_step_of_a_chunk_skipped", "sign_not_decided", "last_step_judged_without_its_neighbour"):
        assert BY_NAME[name]["old"] in search, name
    assert BY_NAME["coset4_doublings_dropped"]["old"] in dlog[dlog.index("ZC_DI pt dlog_start("):dlog.index("ZC_DI bool dlog_search(")]
    assert BY_NAME["fixed_number_of_slots_read"]["old"] in dlog[dlog.index("ZC_DI long dlog_lookup("):dlog.index("ZC_DI bool dlog_y_is(")]
    assert BY_NAME["parity_bit_left_out_of_the_record"]["old"] in dlog[dlog.index("ZC_DI void dlog_build_run("):dlog.index("struct dlog_table {")]
    # the rows ask for every baby step of the small tables, and some table holds a record that linear probing moved two slots or more
    moved = [max(DR.slots_of(DR.table_records(oracle, name, t, c), t)[1]) for name in DR.GENERATORS for t in DR.EMUL_BITS for c in (0, 1)]
    assert max(moved) >= 2 and all(set(range(1 << t)) <= set(DR.found_values(t)) for t in DR.EMUL_BITS)
    # and for a last step of a chunk that matches: m = (C - 1) T + T - 1
    c = DR.plan_constants()["chunk"]
    assert all(((c - 1) << t) + (1 << t) - 1 in DR.found_values(t) for t in DR.EMUL_BITS)


def test_unmutated_copy_passes(built, oracle):
    assert DR.failures(C.CDLL(built[None]), oracle) == []


@pytest.mark.parametrize("name", [m["name"] for m in MUTANTS])
def test_planted_defect_is_killed(built, oracle, name):
    EB.assert_killed(BY_NAME[name], DR.failures(C.CDLL(built[name]), oracle))
