"""CPU tier: defects planted in the generator sets' device code must be caught by the rows of tests/gens_rows.py.

The catalogue below is this feature's own (tests/mutants.py is left as it is).  Per entry the headers and the emulation source
are copied into a temporary directory, the one replacement is applied to the copied header, tests/emul/gens_emul.cpp is built
from the copy with g++ (no sanitizer, no bounds assertions) and GR.failures run on it: at least one check must fail, and the
families `killers` names must be among the failures (where `spared` names some, they must pass).  Every planted defect stays
inside the tables the emulation allocates.  The unmutated copy passes, and every `old` text occurs exactly once in its header.
Nothing is written inside the repository tree."""
import concurrent.futures
import ctypes as C
import glob
import os
import shutil
import subprocess

import pytest

from tests import gens_rows as GR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "dusk_zerocaf_amd", "csrc")
EMUL_DIR = os.path.join(HERE, "emul")
ROCM_INC = "/opt/rocm/include"
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


def make_copy(where, m=None):
    csrc = os.path.join(where, "dusk_zerocaf_amd", "csrc")
    emul = os.path.join(where, "tests", "emul")
    os.makedirs(csrc)
    os.makedirs(emul)
    for f in glob.glob(os.path.join(CSRC, "*.h")):
        shutil.copy(f, csrc)
    shutil.copy(os.path.join(EMUL_DIR, "gens_emul.cpp"), emul)
    if m is not None:
        path = os.path.join(csrc, m["header"])
        with open(path) as f:
            text = f.read()
        assert text.count(m["old"]) == 1, m["name"]
        with open(path, "w") as f:
            f.write(text.replace(m["old"], m["new"]))
    so = os.path.join(where, "libzc_gens.so")
    subprocess.check_call(["g++", "-std=c++17", "-fPIC", "-shared", "-O2", "-D__HIP_PLATFORM_AMD__", "-fno-gnu-unique", "-Wl,-Bsymbolic",
                           "-I" + ROCM_INC, "-o", so, os.path.join(emul, "gens_emul.cpp")])
    return so


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    if not os.path.isdir(ROCM_INC):
        pytest.skip("ROCm headers not present")
    names = [None] + [m["name"] for m in MUTANTS]
    dirs = [str(tmp_path_factory.mktemp(n or "unmutated")) for n in names]
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        out = dict(zip(names, pool.map(lambda a: make_copy(a[0], BY_NAME.get(a[1])), zip(dirs, names))))
    assert not any(p.startswith(ROOT + os.sep) for p in out.values())
    return out


def test_catalogue_is_sound():
    assert len(BY_NAME) == len(MUTANTS) and 4 <= len(MUTANTS)
    for m in MUTANTS:
        text = open(os.path.join(CSRC, m["header"])).read()
        assert text.count(m["old"]) == 1 and m["old"] != m["new"], m["name"]
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
    m = BY_NAME[name]
    failed = GR.failures(C.CDLL(built[name]), oracle)
    assert failed != [], "%s survived" % name
    families = {f.rsplit(" [", 1)[0] for f in failed}
    assert set(m["killers"]) <= families, (name, sorted(families))
    assert not set(m.get("spared", [])) & families, (name, sorted(families))
    for case in m.get("cases", []):
        assert case in failed, (name, case, failed)
    for case in m.get("spared_cases", []):
        assert case not in failed, (name, case, failed)
