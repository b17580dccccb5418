"""CPU tier: the device functions behind the scalar vector ops (zc_scvec.hip.h: scv_block_slice, scv_slice_sum, scv_slice_dot,
scv_cols_fold, scv_pair, the tree, scv_pow_lane; zc_scvec_plan.h: the cut and the grids), built for the host by
tests/emul/scvec_emul.cpp in the plain and the bounds-asserting (-DZC_CHECK_BOUNDS) build.  Every family and every shape of
tests/scvec_rows.py against Python integers; the column and fold bounds at the worst-magnitude rows and at the longest slice a
call can produce; results that depend on the row alone.  The sanitizer run is a stand-alone program (tests/emul/scvec_san.cpp)
replaying a vector file as a child process: nothing sanitized is loaded here."""
import ctypes as C
import struct

import numpy as np
import pytest

from oracle import pymodel as pm
from tests import emul_build as EB
from tests import scvec_rows as R

L = R.L


@pytest.fixture(scope="module", params=["plain", "checked"])
def emul(request):
    so = EB.library("scvec_emul.cpp", checked=request.param == "checked")
    if so is None:
        pytest.skip("ROCm headers not present")
    return R.Emul(C.CDLL(so))


def test_the_rows_are_what_the_issue_asks_for(emul):
    c = emul.constants()
    assert c == {k: R.plan_constants().get(k, c[k]) for k in c} and c["SCV_POW_STAGE_STEPS"] * 256 == R.plan_constants()["SCV_POW_STAGE"]
    for shapes, ths in ((R.row_shapes(), R.rows_thresholds()), (R.pow_shapes(), R.pow_thresholds())):
        assert {n for n, _ in shapes} == {1, 3, 63, 64, 65, 257}
        assert {t for _, t in shapes} >= {0, 1, 2, 3, 7, 8, 31, 32, 33, 64, 65, 511, 512, 513, 16 * (1 << 16) + 5}
        assert all((n, t + d) in shapes for t in ths for n in (1, 3) for d in (0, 1))
    pool = [R.SR.value(w) for w in R.edge_pool()]
    for v in (0, 1, L - 1, L, 2047 * L, 2**249 - 1, 2**249, 2**260 - 1):
        assert v in pool
    assert any(not (np.array(w, dtype=np.uint64) & np.uint64(R.M52)).any() and any(w) for w in R.edge_pool())        # words with only bits >= 2^52 set
    assert all(int(v) < 1 << 249 for v in R.vals(R.fill(3, 7, "random", 1)).ravel()) and (R.fill(2, 3, "worst", 1) == R.ALL_ONES).all()
    xs = [int(v) % L for v in R.vals(R.bases(64, 5))]
    assert {0, 1, L - 1} <= set(xs) and any(1 < min(q for q in range(1, 1000) if pow(x, q, L) == 1 or q == 999) < 999 for x in xs if x > 1 and x != L - 1)
    assert max(R.slice_lengths()) == c["SCV_LONGEST_SLICE"] and {c["SCV_CARRY_EVERY"], c["SCV_CARRY_EVERY"] + 1, c["SCV_NOHI_MAX"], c["SCV_NOHI_MAX"] + 1} <= set(R.slice_lengths())
    kinds = {(op, fam) for op, fam, _, _ in R.cases()}
    assert kinds == {(op, fam) for op in ("sum", "dot", "dot_shared") for fam in R.FAMILIES} | {("powers", "bases")}


@pytest.mark.parametrize("key", R.cases(), ids=lambda k: R.label(*k))
def test_every_family_and_shape_is_the_python_integers(emul, key):
    op, fam, n, terms = key
    c = R.case(*key)
    got = emul.run(op, *c[:-1], terms=terms)
    assert got.shape == c[-1].shape
    bad = np.argwhere((got != c[-1]).any(axis=-1))
    assert len(bad) == 0, bad[:8]
    assert emul.bound_failures() == 0


def test_worst_magnitude_slices_keep_the_column_and_fold_bounds(emul):
    """Every operand 2^260 - 1 under all-ones words: slices around the carry passes, around the nineteenth limb, and the longest
    a call can produce.  The checked build asserts room for a product in every column before it is added, the nineteenth limb
    below 2^29 and the Montgomery reduction's input below 2^522."""
    worst = [R.ALL_ONES] * 5
    for m in R.slice_lengths():
        assert emul.slice_dot(worst, worst, m).tolist() == pm.limbs(m * R.WORST * R.WORST % L), m
        assert emul.slice_sum(worst, m).tolist() == pm.limbs(m * R.WORST % L), m
    top, one = pm.limbs(2**249), pm.limbs(1)                                             # an operand at 2^TOPBIT against the smallest
    for m in (1, 5, 9, 65):
        assert emul.slice_dot(top, one, m).tolist() == pm.limbs(m * 2**249 % L) and emul.slice_dot(top, worst, m).tolist() == pm.limbs(m * 2**249 * R.WORST % L)
    assert emul.bound_failures() == 0


def test_results_depend_on_the_row_alone(emul):
    """The same row among other rows, in another batch size, under another cut of the plan (a row of 300 terms alone and as the
    head of a longer computation split by hand): limb for limb the same."""
    a, b, want = R.case("dot", "edges", 65, 33)
    for i in (0, 31, 64):
        assert np.array_equal(emul.run("dot", a[i:i + 1], b[i:i + 1])[0], want[i]) and np.array_equal(emul.run("sum", a[i:i + 1])[0], R.sum_expected(a[i:i + 1])[0])
    big = R.fill(1, 40000, "random", 3)
    parts = [emul.run("sum", big[:, lo:lo + 1000])[0] for lo in range(0, 40000, 1000)]
    again = emul.run("sum", np.array(parts, dtype=np.uint64).reshape(1, 40, 5))[0]
    assert np.array_equal(again, emul.run("sum", big)[0])
    x, rows = R.case("powers", "bases", 65, 33)
    assert np.array_equal(emul.run("powers", x[7:8], terms=513)[0, :33], rows[7])


def test_the_whole_tier_passes_as_the_mutant_test_runs_it(emul):
    assert R.failures(emul) == []


def test_stand_alone_program_under_asan_and_ubsan(tmp_path):
    """tests/emul/scvec_san.cpp with -fsanitize=address,undefined -fno-sanitize-recover=all: inputs and outputs in heap blocks of
    exactly their size; its exit status is the verdict."""
    exe = EB.sanitizer_program("scvec_san.cpp", tmp_path)
    parts, rows = [], 0
    for key in [("sum", "edges", 65, 7), ("sum", "random", 1, 32769), ("dot", "edges", 63, 3), ("dot", "worst", 3, 1025), ("dot", "random", 3, 49153), ("dot_shared", "edges", 257, 33),
                ("dot_shared", "random", 3, 1025), ("sum", "random", 64, 0), ("powers", "bases", 65, 33), ("powers", "bases", 3, 257), ("powers", "bases", 1, 16385)]:
        op, fam, n, t = key
        c = R.case(*key)
        parts.append(struct.pack("<3Q", ("sum", "dot", "dot_shared", "powers").index(op), n, t) + b"".join(np.ascontiguousarray(x).tobytes() for x in c))
        rows += n
    blob = b"".join(parts) + struct.pack("<Q", 4)
    EB.assert_clean(EB.run_vectors(exe, blob, tmp_path, "vectors.bin"), "%d records, %d rows match" % (len(parts), rows))
    bad = bytearray(blob)
    bad[-16] ^= 1                                                                       # the last record's last expected limb
    EB.assert_caught(EB.run_vectors(exe, bad, tmp_path, "wrong.bin"), "record %d: row 0:" % (len(parts) - 1))
