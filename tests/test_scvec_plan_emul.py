"""CPU tier: the host plan of the scalar vector ops (dusk_zerocaf_amd/csrc/zc_scvec_plan.h, built with g++ alone through
tests/emul/scvec_plan_emul.cpp -- no HIP header) over a grid of (n, terms) including the limits: every record of a row belongs to
exactly one (row, slice, step) and every power to one (row, lane, step); the grids cover their rows; the workspace holds the
partials; the 2^31 limit is decided without forming the product; and the shape list of tests/scvec_rows.py reaches every form
and both sides of every threshold."""
import ctypes as C
import os
import re

import pytest

from tests import emul_build as EB
from tests import scvec_rows as R

ULL = C.c_ulonglong
TERMS = sorted(set(list(range(0, 70)) + [127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097, 16383, 16384, 16385, 32767, 32768, 32769, 49151, 49152,
                                        49153, 65535, 65536, 65537, 262143, 262144, 262145, R.BIG_ROW, (1 << 22) - 1, 1 << 22, (1 << 22) + 1, 1 << 24, (1 << 24) + 77, (1 << 31) - 1]))
NS = [1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000]


@pytest.fixture(scope="module")
def plan():
    so = EB.library("scvec_plan_emul.cpp", flags=EB.STRICT)
    if so is None:
        pytest.skip("ROCm headers not present")
    lib = C.CDLL(so)
    lib.plan_scvec_slice_len.restype = ULL
    lib.plan_scvec_slice_len.argtypes = [ULL, ULL, ULL]
    lib.plan_scvec_too_large.argtypes = [ULL, ULL]
    return lib


def constants(lib):
    out = (ULL * 15)()
    lib.plan_scvec_constants(out)
    names = ("block", "index_limit", "partial_words", "stage", "block_terms_max", "p256_max", "two_row_terms", "max_bpr", "carry_every", "nohi_max", "longest_slice", "pow_stage",
             "pow_stage_steps", "pow_g256_max", "pow_g4096_max")
    return dict(zip(names, map(int, out)))


def rows_plan(lib, n, terms):
    out = (ULL * 9)()
    lib.plan_scvec(ULL(n), ULL(terms), out)
    return dict(zip(("parts", "steps", "form", "rows_per_block", "blocks_per_row", "grid1", "grid2", "partials", "workspace_bytes"), map(int, out)))


def pow_plan(lib, n, terms):
    out = (ULL * 5)()
    lib.plan_scvec_pow(ULL(n), ULL(terms), out)
    return dict(zip(("group", "steps", "rows_per_block", "blocks_per_row", "grid"), map(int, out)))


def test_plan_header_is_host_only_and_its_constants_are_the_ones_the_rows_read(plan):
    text = open(os.path.join(EB.CSRC, "zc_scvec_plan.h")).read()
    code = re.sub(r"//[^\n]*", "", text)
    assert re.findall(r"#include\s+(\S+)", text) == ["<cstddef>", "<cstdint>"] and "__device__" not in code and "hip" not in code.lower()
    c, rc = constants(plan), R.plan_constants()
    assert (c["block"], c["index_limit"], c["partial_words"]) == (256, 1 << 31, 10)
    for k in ("stage", "block_terms_max", "p256_max", "two_row_terms", "max_bpr", "carry_every", "nohi_max", "pow_stage", "pow_g256_max", "pow_g4096_max"):
        assert c[k] == rc["SCV_" + k.upper()], k
    assert c["pow_stage_steps"] * 256 == c["pow_stage"] and c["longest_slice"] == -(-((1 << 31) - 1) // (256 * c["max_bpr"])) == max(R.slice_lengths())
    # seven products of 260-bit operands and a carried-in limb fit a column; up to nohi_max products stay below 2^522
    assert c["carry_every"] * 9 * (1 << 58) + (1 << 29) < 1 << 64 <= (c["carry_every"] + 1) * 9 * (1 << 58) + (1 << 29)
    assert c["nohi_max"] * (1 << 520) <= 1 << 522 < (c["nohi_max"] + 1) * (1 << 520)
    assert c["longest_slice"] * (1 << 520) < 1 << 551                                   # the nineteenth limb stays below 2^29


@pytest.mark.parametrize("terms", TERMS)
def test_every_record_belongs_to_exactly_one_row_slice_and_step(plan, terms):
    c = constants(plan)
    for n in NS:
        if plan.plan_scvec_too_large(n, terms):
            continue
        p = rows_plan(plan, n, terms)
        P, steps = p["parts"], p["steps"]
        assert steps == -(-terms // P)
        lens = [int(plan.plan_scvec_slice_len(terms, P, s)) for s in ({0, 1, P // 2, P - 1} if P > 4096 else range(P))]
        assert max(lens) == steps or terms == 0
        if P <= 4096:
            assert sum(lens) == terms                                                   # slice s holds s, s + P, ...: a partition of 0 .. terms - 1
            assert all(ln == len(range(s, terms, P)) for s, ln in enumerate(lens))
        else:
            assert P * (steps - 1) < terms <= P * steps
        if p["form"] == 0:                                                              # the block form: at most four records per lane, the block fits the stage
            assert terms <= c["block_terms_max"] and P in (1, 4, 16, 64, 256) and steps <= c["nohi_max"] and (P == 1 or terms > c["nohi_max"] * P // 4)
            assert p["rows_per_block"] == 256 // P and p["blocks_per_row"] == 1 and p["rows_per_block"] * terms <= c["stage"]
            assert p["grid1"] == -(-n // p["rows_per_block"]) and p["grid1"] * p["rows_per_block"] >= n > (p["grid1"] - 1) * p["rows_per_block"]
            assert (p["grid2"], p["partials"], p["workspace_bytes"]) == (0, 0, 0)
        elif p["form"] == 1:
            assert c["block_terms_max"] < terms <= c["p256_max"] and P == 256 and (p["rows_per_block"], p["blocks_per_row"], p["grid1"]) == (1, 1, n)
            assert (p["grid2"], p["partials"], p["workspace_bytes"]) == (0, 0, 0)
        else:
            bpr = p["blocks_per_row"]
            assert p["form"] == 2 and terms > c["p256_max"] and P == 256 * bpr and 2 <= bpr <= c["max_bpr"] and bpr == min(c["max_bpr"], -(-terms // c["two_row_terms"]))
            assert p["rows_per_block"] == 1 and p["grid1"] == n * bpr == p["partials"] and p["grid2"] == n
            assert p["workspace_bytes"] == p["partials"] * c["partial_words"] * 4 and p["grid1"] < 1 << 31
            assert steps <= c["longest_slice"]


@pytest.mark.parametrize("terms", TERMS)
def test_every_power_belongs_to_exactly_one_row_lane_and_step(plan, terms):
    c = constants(plan)
    for n in NS:
        if plan.plan_scvec_too_large(n, terms):
            continue
        p = pow_plan(plan, n, terms)
        G, steps = p["group"], p["steps"]
        assert G & (G - 1) == 0 and 1 <= G <= max(terms, 1) and steps == -(-terms // G)
        assert G * (steps - 1) < terms <= G * steps or terms == 0                       # j = l + k G, l < G, k < steps: every j once
        if G < 256:
            assert steps <= c["pow_stage_steps"] and p["rows_per_block"] == 256 // G and p["blocks_per_row"] == 1
            assert p["rows_per_block"] * terms <= c["pow_stage"]                        # the workgroup's block fits the staging area
            assert p["grid"] == -(-n // p["rows_per_block"])
        else:
            assert p["rows_per_block"] == 1 and p["blocks_per_row"] == G // 256 and p["grid"] == n * G // 256 < 1 << 31
        assert n * G < 1 << 31 or terms == 0


def test_the_limit_is_decided_without_the_product(plan):
    for terms in (0, 1, 2, 3, 7, 1000, 65536, 65537, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, 1 << 40, (1 << 63) + 5, (1 << 64) - 1):
        for n in (0, 1, 2, 3, 32767, 32768, 65535, 65536, (1 << 31) - 1, 1 << 31, 1 << 33, (1 << 63) + 9, (1 << 64) - 1):
            assert bool(plan.plan_scvec_too_large(n, terms)) == (n * terms >= 1 << 31), (n, terms)
        if terms:
            edge = -(-(1 << 31) // terms)
            assert plan.plan_scvec_too_large(edge, terms) and (edge == 0 or not plan.plan_scvec_too_large(edge - 1, terms))


def test_the_shape_list_reaches_every_form_and_both_sides_of_every_threshold(plan):
    c = constants(plan)
    rows, pows = R.row_shapes(), R.pow_shapes()
    for shapes in (rows, pows):
        assert {n for n, _ in shapes} >= {1, 3, 63, 64, 65, 257} and {t for _, t in shapes} >= set(R.GENERAL_TERMS) | {R.BIG_ROW}
    assert R.BIG_ROW == 16 * (1 << 16) + 5 and (1, R.BIG_ROW) in rows and (1, R.BIG_ROW) in pows
    # sums and dot products: the thresholds are where parts, the form or the fold's nineteenth limb change
    seen = {(rows_plan(plan, n, t)["form"], min(rows_plan(plan, n, t)["parts"], 512)) for n, t in rows}
    assert seen == {(0, 1), (0, 4), (0, 16), (0, 64), (0, 256), (1, 256), (2, 512)}
    changes = [t for t in range(1, 40000) if (rows_plan(plan, 1, t)["parts"], rows_plan(plan, 1, t)["form"]) != (rows_plan(plan, 1, t + 1)["parts"], rows_plan(plan, 1, t + 1)["form"])]
    assert changes == R.rows_thresholds()[:6] and R.rows_thresholds()[0] == c["nohi_max"] and R.rows_thresholds()[4] == c["block_terms_max"]
    for th in R.rows_thresholds():
        for n in (1, 3):
            assert (n, th) in rows and (n, th + 1) in rows, th
    assert rows_plan(plan, 1, c["block_terms_max"])["steps"] == c["nohi_max"] < rows_plan(plan, 1, c["block_terms_max"] + 1)["steps"]      # the nineteenth limb: both sides
    assert any(rows_plan(plan, n, t)["form"] and rows_plan(plan, n, t)["steps"] > 2 * c["carry_every"] for n, t in rows)                    # slices with carry passes
    bprs = {rows_plan(plan, n, t)["blocks_per_row"] for n, t in rows}
    assert {1, 3, 4} <= bprs and any(b % 2 and b > 3 for b in bprs)                   # trees with an odd level at the top and further down
    # powers: every group size, both sides of every change
    changes = [t for t in range(1, 300000) if pow_plan(plan, 1, t)["group"] != pow_plan(plan, 1, t + 1)["group"]]
    assert changes == R.pow_thresholds()
    for th in changes:
        for n in (1, 3):
            assert (n, th) in pows and (n, th + 1) in pows, th
    assert {pow_plan(plan, n, t)["group"] for n, t in pows if t} == {1, 4, 16, 64, 256, 4096, 65536}
    assert any(pow_plan(plan, n, t)["steps"] > c["pow_stage_steps"] and t % 256 for n, t in pows)      # more than one flush, a ragged last step
