"""CPU tier: the MSM host plans (dusk_zerocaf_amd/csrc/zc_msm_plan.h) against a recorded table.

tests/emul/msm_plan_emul.cpp includes that header alone -- plain g++, no HIP -- and, for one call of zc_msm, zc_msm_batch,
zc_msm_bases_create + zc_msm_fixed or the sort test hook, runs the index-limit checks and the plan in the host code's order
and returns every field: window bits and count, record form and stride, run and segment lengths, list entries, buckets,
segments, level-0 lanes, the window groups, the key sort's passes and table, the bytes of the workspace, and which limit a
call past one breaks.  tests/golden/msm_plan_table.json holds the expected rows over a grid of the sizes and knobs at which
the rules branch (grid() below).

How the committed table was made: NOT from this header.  The three plan structs, the two window searches, the two limit
checks and the four workspace carves that zerocaf_hip.hip held before the header existed (commit 472c308) were lifted
verbatim into a throwaway program with the same C interface, and that program wrote the table; the header must reproduce it.
After an intentional plan change, `python -m tests.test_msm_plan_emul` rewrites the table from the current header -- review
the diff of the table like code."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

from tests import emul_build as EB
from tests.emul_build import EMUL_DIR, HERE, ROOT

TABLE = os.path.join(HERE, "golden", "msm_plan_table.json")

FIELDS = (["limit", "buckets", "c", "W", "affine", "rec_bytes", "T", "TE", "seg", "m", "nb", "nseg", "nl0", "G"] +
          ["gw%d" % g for g in range(4)] + ["gT%d" % g for g in range(4)] + ["gseg%d" % g for g in range(4)] +
          ["bad_groups", "sort_passes", "sort_packed", "sort_big", "sort_table_words", "sort_tile", "sort_G", "sort_ncols", "sort_idx_bits"] +
          ["sort_bits%d" % i for i in range(4)] + ["workspace_bytes"])
LIMITS = {0: "none", 1: "31-bit record indices", 2: "32-bit pair indices", 3: "32-bit bucket keys"}
KINDS = {0: "zc_msm(n pairs; arg = points 16-byte aligned)", 1: "zc_msm_batch(batch instances of n pairs; arg = aligned)",
         2: "zc_msm_bases_create(n bases, window_bits = arg) + zc_msm_fixed(batch vectors)", 3: "zc_test_msm_sort(n scalars, c = arg)"}
KNOB_NAMES = ["window", "affine", "groups", "sort_packed", "sort_big", "sort_g", "run", "run_edges", "seg"]
KNOB_SETS = [
    {},
    {"window": 8},
    {"run": 16, "seg": 4, "sort_packed": 0},
    {"groups": [17, 4], "window": 13},            # 21 windows: a valid split
    {"groups": [10, 11]},                         # adds up to 21: every shard with another window count reports bad_groups
    {"seg": 64, "window": 6},                     # 32 buckets per window: the segment is cut to 32
    {"run_edges": 5},                             # rounded down to even
    {"window": 17},                               # 16 windows: the only power of two, for the cases that sit exactly on a limit
]


def knob_array(ks):
    g = list(ks.get("groups", []))
    v = [ks.get("window", 0), ks.get("affine", -1), len(g)] + (g + [0] * 4)[:4] + [ks.get("sort_packed", -1), ks.get("sort_big", -1),
                                                                                     ks.get("sort_g", 0), ks.get("run", 0), ks.get("run_edges", 0), ks.get("seg", 0)]
    assert set(ks) <= set(KNOB_NAMES)
    return (C.c_int32 * 13)(*v)


def around(es):
    return list(dict.fromkeys(x for e in es for x in ((1 << e) - 1, 1 << e, (1 << e) + 1)))     # (2^0 + 1 = 2^1, 2^1 + 1 = 2^2 - 1: once)


def grid():
    """[kind, n, batch, arg, knob set] -- a few hundred cases; every threshold of the rules has its 2^e - 1, 2^e, 2^e + 1."""
    rows = []
    # zc_msm: e = 0 .. 26 crosses the bucket threshold (2^12), affine records (2^17), c = 17 (2^19, 2^20), the default window
    # groups (2^21 .. 2^22), the big sort tiles (2^22) and the 256-entry runs (m >= 2^27)
    for n in around(range(27)):
        rows.append([0, n, 1, 1, 0])
    for n in around(range(16, 27, 2)) + around([21]):
        rows.append([0, n, 1, 0, 0])                                                    # unaligned points: never affine
    for ks in range(1, 7):
        for n in around([12, 16, 20, 21, 22, 24]):
            rows.append([0, n, 1, 1, ks])
    rows += [[0, (1 << 31) - 1, 1, 1, 0], [0, 1 << 31, 1, 1, 0], [0, 1 << 28, 1, 1, 0], [0, 1 << 28, 1, 1, 7], [0, (1 << 28) - 1, 1, 1, 7]]
    # zc_msm_batch: the bucket threshold (64), the widths the cost search picks, affine from batch n = 2^17 on
    for batch in (2, 3, 16, 1000):
        for n in around([0, 6, 9, 12, 15, 17, 20])[1:]:
            rows.append([1, n, batch, 1, 0])
        for n in around([12, 17]):
            rows.append([1, n, batch, 0, 0])
        for ks in range(1, 7):
            rows.append([1, 4096, batch, 1, ks])
    # fixed-base: every window_bits, 1 / 7 / 256 vectors
    for wb in (0, 5, 9, 16, 22):
        for vectors in (1, 7, 256):
            for n in (1, 64, 4097, 1 << 16, (1 << 20) + 1, 1 << 24):
                rows.append([2, n, vectors, wb, 0])
    for ks in (2, 5, 6):
        for vectors in (1, 7, 256):
            rows.append([2, 1 << 16, vectors, 0, ks])
    # the sort hook
    for c in (5, 10, 11, 16, 19, 20, 22):
        for n in (1, 4097, 1 << 16, (1 << 22) + 1):
            rows.append([3, n, 1, c, 0])
    rows += [[3, 1 << 16, 1, 13, 2], [3, 1 << 28, 1, 17, 0], [3, (1 << 28) - 1, 1, 17, 0]]
    # on the index limits and one below: n batch = 2^31; n batch W = 2^32 and batch W 2^(c-1) = 2^32 (W = 16); fixed-base n W = 2^31
    for n, batch, ks in ((1 << 16, 1 << 15, 0), (1 << 16, (1 << 15) - 1, 0), (1, 1 << 31, 0), (1 << 31, 2, 0), (1 << 14, 1 << 14, 7), (1 << 14, (1 << 14) - 1, 7),
                         ((1 << 14) - 1, 1 << 14, 7), (64, 4096, 7), (64, 4095, 7), (1 << 20, 2048, 0), (1 << 20, 2047, 0)):
        rows.append([1, n, batch, 1, ks])
    for n, vectors, wb in ((1 << 27, 1, 17), ((1 << 27) - 1, 1, 17), ((1 << 27) - 1, 7, 17), (1 << 16, 4096, 17), (1 << 16, 4095, 17), (1 << 10, 4096, 21),
                           (1 << 10, 4095, 21), (64, 1 << 29, 5), (1 << 40, 1, 0)):
        rows.append([2, n, vectors, wb, 0])
    return rows


def build_emul():
    so = EB.library("msm_plan_emul.cpp", sanitize=bool(os.environ.get("ZC_EMUL_SANITIZE")), flags=EB.STRICT)
    if so is None:
        pytest.skip("ROCm headers not present")
    lib = C.CDLL(so)
    lib.emul_msm_plan.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    assert lib.emul_msm_plan_fields() == len(FIELDS)
    return lib


def run_case(lib, case):
    kind, n, batch, arg, ks = case
    out = (C.c_int64 * len(FIELDS))()
    assert lib.emul_msm_plan(kind, n, batch, arg, knob_array(KNOB_SETS[ks]), out) == 0
    return list(out)


@pytest.fixture(scope="module")
def emul():
    return build_emul()


@pytest.fixture(scope="module")
def table():
    return json.load(open(TABLE))


def test_table_is_the_grid(table):
    assert table["fields"] == FIELDS and table["knob_sets"] == KNOB_SETS
    assert [r[:5] for r in table["rows"]] == grid()
    assert 300 <= len(table["rows"]) <= 800 and os.path.getsize(TABLE) <= os.path.getsize(os.path.join(HERE, "golden", "ref_kats.json"))


def test_every_plan_field_matches_the_recorded_table(emul, table):
    bad = []
    for row in table["rows"]:
        got = run_case(emul, row[:5])
        if got != row[5:]:
            bad.append((row[:5], {f: (w, g) for f, w, g in zip(FIELDS, row[5:], got) if w != g}))
    assert not bad, "%d of %d cases differ (field: (recorded, header)), first: %r" % (len(bad), len(table["rows"]), bad[:3])


def test_table_covers_the_branches(table):
    """The grid is only worth its rows if the recorded outcomes really differ where the rules branch."""
    col = {f: i + 5 for i, f in enumerate(FIELDS)}
    rows = table["rows"]
    by = lambda kind, **kw: [r for r in rows if r[0] == kind and all(r[col[f]] == v for f, v in kw.items())]
    assert {r[col["limit"]] for r in rows if r[0] == 1} == {0, 1, 2, 3} and {r[col["limit"]] for r in rows if r[0] == 2} == {0, 1, 2, 3}
    assert {r[col["limit"]] for r in rows if r[0] == 0} == {0, 1, 2} and {r[col["limit"]] for r in rows if r[0] == 3} == {0, 2}
    assert by(0, G=3, gw0=9, gw1=4, gw2=3) and by(0, G=2, gw0=17, gw1=4) and by(0, bad_groups=21) and by(0, c=17, W=16) and by(0, T=256)
    assert by(0, buckets=0) and by(0, affine=0, buckets=1) and by(0, affine=1) and by(0, sort_big=1) and by(0, sort_packed=1) and by(0, sort_packed=0, sort_passes=2)
    assert by(0, seg=32, c=6) and by(0, TE=4) and by(0, TE=8) and by(0, seg=4, T=16)
    assert by(1, buckets=0) and by(1, buckets=1, affine=1) and by(1, buckets=1, affine=0) and {r[col["sort_passes"]] for r in by(3, limit=0)} == {1, 2, 3}
    assert {r[col["c"]] for r in by(2, limit=0)} >= {5, 9, 16, 22} and len({r[col["c"]] for r in by(2, limit=0) if r[3] == 0}) >= 3


def test_msm_plan_emul_under_asan_and_ubsan():
    """The same table with the driver under AddressSanitizer + UBSan: shifts, casts and the saturating products at the limits."""
    if os.environ.get("ZC_EMUL_SANITIZE"):
        pytest.skip("already inside the sanitizer run")
    rt = []
    for name in ("libasan.so", "libubsan.so"):
        path = subprocess.run(["gcc", "-print-file-name=" + name], capture_output=True, text=True).stdout.strip()
        if not (os.path.isabs(path) and os.path.exists(path)):
            pytest.skip("gcc's sanitizer runtimes are not installed")
        rt.append(path)
    preload = ":".join(rt + [x for x in [os.environ.get("LD_PRELOAD")] if x])
    env = dict(os.environ, LD_PRELOAD=preload, ZC_EMUL_SANITIZE="1",
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "recorded_table"],
                         capture_output=True, text=True, cwd=ROOT, env=env, timeout=600)
    tail = (out.stdout + out.stderr)[-3000:]
    assert out.returncode == 0 and " passed" in out.stdout and "runtime error" not in tail and "AddressSanitizer" not in tail, tail
    assert os.path.exists(os.path.join(EMUL_DIR, "libzc_msm_plan_san.so"))


def write_table(lib, path):
    rows = [case + run_case(lib, case) for case in grid()]
    with open(path, "w") as f:
        f.write('{"kinds": %s,\n "limits": %s,\n "knob_sets": %s,\n "case": ["kind", "n", "batch", "arg", "knob_set"],\n "fields": %s,\n "rows": [\n' %
                (json.dumps(KINDS), json.dumps(LIMITS), json.dumps(KNOB_SETS), json.dumps(FIELDS)))
        f.write(",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in rows))
        f.write("\n ]}\n")
    return len(rows)


if __name__ == "__main__":
    print("%d rows -> %s" % (write_table(build_emul(), TABLE), TABLE))
