"""CPU tier: the host plan of the point sums (dusk_zerocaf_amd/csrc/zc_sum_plan.h, built with g++ alone through
tests/emul/sum_rows_emul.cpp) against the Python restatement of tests/sum_rows.py and against the header's text: parts(terms),
the grids and the workspace of every form, the refusal limit."""
import ctypes as C
import os
import re

import pytest

from tests import emul_build as EB
from tests import sum_rows as SR
from tests.emul_build import ROOT

GROUP, TWO = 0, 1


@pytest.fixture(scope="module")
def emul():
    so = EB.library("sum_rows_emul.cpp")
    if so is None:
        pytest.skip("ROCm headers not present")
    return SR.Emul(C.CDLL(so))


def _edges():
    out = set(range(10001))
    for k in range(1, 32):
        out |= {(1 << k) - 1, 1 << k, (1 << k) + 1}
    return sorted(t for t in out if t < 1 << 31)


def test_parts_is_the_python_restatement_a_power_of_two_and_never_above_terms(emul):
    for t in _edges():
        p = emul.parts(t)
        assert p == SR.parts(t), t
        assert p & (p - 1) == 0 and 1 <= p <= max(t, 1) and p <= 1 << 16
        if p > 1:
            assert 16 * p <= t and (p == 1 << 16 or 32 * p > t)                           # every slice holds at least 16 points
    assert emul.parts((1 << 31) - 1) == 1 << 16


def test_constants_are_the_headers(emul):
    c = emul.constants()
    assert c == dict(serial_max=SR.SERIAL_MAX, min_slice=SR.MIN_SLICE, max_parts=SR.MAX_PARTS, block=SR.BLOCK, partial_words=40, index_limit=1 << 31)
    text = " ".join(open(os.path.join(ROOT, "include", "zerocaf_hip_ext_sum_rows.h")).read().replace("\n *", "\n").split())
    for word in ("P = 1 for terms <= 32", "largest power of two with 16 * P <= terms", "at most 2^16", "more than 8191 terms"):
        assert word in text, word
    assert re.search(r"n \* terms >= 2\^31", text)


def test_the_forms_their_grids_and_the_workspace(emul):
    for t in [0, 1, 2, 32, 33, 47, 511, 512, 4095, 4096, 8191, 8192, 8197, 1 << 16, (1 << 20) - 1, 1 << 20, 1 << 24, (1 << 31) - 1]:
        for n in (1, 2, 3, 255, 256, 257, 1000, 1 << 20):
            if t and n * t >= 1 << 31:
                assert emul.too_large(n, t)
                continue
            assert not emul.too_large(n, t)
            p = emul.plan(n, t)
            P = SR.parts(t)
            assert p["parts"] == P and p["steps"] == -(-t // P) == (emul.fold_steps(t, P) if t else 0)       # the kernels' own count
            if P <= SR.BLOCK:
                assert p["form"] == GROUP and p["rows_per_block"] == SR.BLOCK // P and p["blocks_per_row"] == 1
                assert p["grid1"] * p["rows_per_block"] >= n > (p["grid1"] - 1) * p["rows_per_block"]
                assert p["grid2"] == 0 and p["partials"] == 0 and p["workspace_bytes"] == 0
            else:
                assert p["form"] == TWO and p["rows_per_block"] == 1 and p["blocks_per_row"] * SR.BLOCK == P and 2 <= p["blocks_per_row"] <= SR.BLOCK
                assert p["grid1"] == n * p["blocks_per_row"] == p["partials"] and p["grid2"] == n
                assert p["workspace_bytes"] == p["partials"] * 40 * 4                     # every partial the first kernel writes
            assert p["grid1"] < 1 << 31
    assert emul.plan(3, 4096)["form"] == GROUP and emul.plan(3, 8191)["form"] == GROUP and emul.plan(3, 8192)["form"] == TWO


def test_the_refusal_limit_is_n_times_terms_at_2_to_31(emul):
    for t in (1, 2, 3, 7, 1000, 65537, (1 << 31) - 1, 1 << 31, 1 << 40):
        edge = -(-(1 << 31) // t)
        assert emul.too_large(edge, t) and emul.too_large(edge + 1, t) and not emul.too_large(edge - 1, t)
    for n in (0, 1, 1 << 31, 1 << 40):
        assert not emul.too_large(n, 0)
