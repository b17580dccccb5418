"""CPU tier: defects planted in fp_mul_d must be caught by the vectors of tests/fe_muld_rows.py.

The catalogue below is this routine's own (tests/mutants.py is left as it is).  Per entry the headers and the emulation sources
are copied into a temporary directory, the one replacement is applied to the copied header, tests/emul/fe_muld_emul.cpp is
built from the copy with g++ (no sanitizer, no bounds assertions) and FM.failures run on it: at least one input must fail,
and where `killers` names inputs, those must be among the failures.  The unmutated copy passes, and every `old` text
occurs exactly once in its header.  Nothing is written inside the repository tree."""
import concurrent.futures
import ctypes as C
import glob
import os
import shutil
import subprocess

import pytest

from tests import fe_muld_rows as FM

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "dusk_zerocaf_amd", "csrc")
EMUL_DIR = os.path.join(HERE, "emul")
ROCM_INC = "/opt/rocm/include"
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


def make_copy(where, m=None):
    csrc = os.path.join(where, "dusk_zerocaf_amd", "csrc")
    emul = os.path.join(where, "tests", "emul")
    os.makedirs(csrc)
    os.makedirs(emul)
    for f in glob.glob(os.path.join(CSRC, "*.h")):
        shutil.copy(f, csrc)
    shutil.copy(os.path.join(EMUL_DIR, "fe_muld_emul.cpp"), emul)
    if m is not None:
        path = os.path.join(csrc, m["header"])
        with open(path) as f:
            text = f.read()
        assert text.count(m["old"]) == 1, m["name"]
        with open(path, "w") as f:
            f.write(text.replace(m["old"], m["new"]))
    so = os.path.join(where, "libzc_fe_muld.so")
    subprocess.check_call(["g++", "-std=c++17", "-fPIC", "-shared", "-O2", "-D__HIP_PLATFORM_AMD__", "-fno-gnu-unique", "-Wl,-Bsymbolic",
                           "-I" + ROCM_INC, "-o", so, os.path.join(emul, "fe_muld_emul.cpp")])
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
    assert len(BY_NAME) == len(MUTANTS)
    for m in MUTANTS:
        text = open(os.path.join(CSRC, m["header"])).read()
        assert text.count(m["old"]) == 1 and m["old"] != m["new"], m["name"]


def test_unmutated_copy_passes(built, oracle):
    assert FM.failures(C.CDLL(built[None]), oracle) == []


@pytest.mark.parametrize("name", [m["name"] for m in MUTANTS])
def test_planted_defect_is_killed(built, oracle, name):
    failed = FM.failures(C.CDLL(built[name]), oracle)
    assert failed != [], "%s survived" % name
    labels = {f.rsplit(" [", 1)[0] for f in failed}
    assert set(BY_NAME[name]["killers"]) <= labels, (name, sorted(labels)[:20])
