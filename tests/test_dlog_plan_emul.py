"""CPU tier: the host plan of the bounded discrete logs (dusk_zerocaf_amd/csrc/zc_dlog_plan.h, built with g++ alone through
tests/emul/dlog_plan_emul.cpp -- no HIP header) against a Python restatement and the public header's text: sizes, the slices of
every (bound, table_bits) edge, the slot array's layout, and the refusal of a record that occurs twice."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import dlog_rows as DR
from tests import emul_build as EB
from tests.emul_build import ROOT

EMPTY = DR.EMPTY
ULL = C.c_ulonglong


@pytest.fixture(scope="module")
def plan():
    so = EB.library("dlog_plan_emul.cpp", flags=EB.STRICT)
    if so is None:
        pytest.skip("ROCm headers not present")
    lib = C.CDLL(so)
    for name in ("plan_dlog_steps", "plan_dlog_launches", "plan_dlog_offset_word", "plan_dlog_home"):
        getattr(lib, name).restype = ULL
    lib.plan_dlog_tag.restype = C.c_uint
    lib.plan_dlog_build_slots.restype = C.c_long
    lib.plan_dlog_find.restype = C.c_long
    return lib


def constants(lib):
    out = (ULL * 11)()
    lib.plan_dlog_constants(out)
    names = ("min_bits", "max_bits", "max_steps", "chunk", "steps_per_launch", "max_launches", "block", "record_bytes", "setup_stride", "setup_w", "setup_words")
    return dict(zip(names, list(out)))


def slice_of(lib, bound, t, k):
    out = (ULL * 3)()
    lib.plan_dlog_slice(ULL(bound), t, ULL(k), out)
    return tuple(out)


def test_constants_are_the_public_headers_and_what_the_rows_read(plan):
    c = constants(plan)
    text = open(os.path.join(ROOT, "include", "zerocaf_hip_dlog.h")).read()
    for name, key in (("ZC_DLOG_MIN_BITS", "min_bits"), ("ZC_DLOG_MAX_BITS", "max_bits"), ("ZC_DLOG_MAX_STEPS", "max_steps")):
        assert "#define %s %d" % (name, c[key]) in text
    assert (c["min_bits"], c["max_bits"], c["max_steps"], c["steps_per_launch"], c["record_bytes"]) == (4, 22, 65536, 1024, 32)
    assert c["max_launches"] * c["steps_per_launch"] == c["max_steps"] and c["steps_per_launch"] % c["chunk"] == 0 and c["chunk"] >= 2
    assert c["setup_words"] == c["setup_stride"] * (c["setup_w"] + c["max_launches"]) and c["setup_stride"] >= 27
    read = DR.plan_constants()                                                          # the text parser of tests/dlog_rows.py sees the same values
    assert all(read[k] == c[k] for k in read)
    for k in range(c["max_launches"]):
        assert plan.plan_dlog_offset_word(ULL(k)) == c["setup_stride"] * (c["setup_w"] + k)


def test_sizes(plan):
    c = constants(plan)
    for t in range(c["min_bits"], c["max_bits"] + 1):
        out = (ULL * 4)()
        plan.plan_dlog_sizes(t, out)
        assert tuple(out) == (1 << t, 2 << t, 48 << t, (1 << t) // c["chunk"]) and out[3] * c["chunk"] == 1 << t
    assert [t for t in range(0, 40) if plan.plan_dlog_bits_ok(t)] == list(range(4, 23))


def test_slices_cover_every_m_below_the_bound_once_and_no_launch_exceeds_1024_steps(plan):
    c = constants(plan)
    S, Ck = c["steps_per_launch"], c["chunk"]
    for t in (4, 5, 9, 16, 22):
        T = 1 << t
        top = c["max_steps"] << t
        assert not plan.plan_dlog_bound_ok(ULL(0), t) and plan.plan_dlog_bound_ok(ULL(1), t) and plan.plan_dlog_bound_ok(ULL(top), t) and not plan.plan_dlog_bound_ok(ULL(top + 1), t)
        assert not plan.plan_dlog_bound_ok(ULL((1 << 64) - 1), t)
        bounds = {1, 2, T - 1, T, T + 1, Ck * T, Ck * T + 1, S * T - 1, S * T, S * T + 1, S * T + 3 * T + 5, 2 * S * T, 2 * S * T + 1, top - 1, top}
        for bound in sorted(b for b in bounds if 1 <= b <= top):
            steps = -(-bound // T)
            launches = -(-steps // S)
            assert plan.plan_dlog_steps(ULL(bound), t) == steps and plan.plan_dlog_launches(ULL(bound), t) == launches <= c["max_launches"]
            covered = 0
            for k in range(launches):
                first, n, chunks = slice_of(plan, bound, t, k)
                assert first == k * S == covered and 1 <= n <= S and chunks == -(-n // Ck) and chunks * Ck <= S
                covered += n
            assert covered == steps and (steps - 1) * T < bound <= steps * T


def test_the_slot_array_is_the_python_restatement(plan):
    rng = np.random.default_rng(DR.SEED + 40)
    for t in (4, 6, 10):
        records = rng.integers(0, 1 << 63, size=(1 << t, 4), dtype=np.uint64)
        records[3, 0] = records[1, 0]                                                   # equal low words: the same home and tag, another record
        records[5, 0] = records[1, 0]
        slots = np.zeros(2 << t, dtype=np.uint64)
        assert plan.plan_dlog_build_slots(slots.ctypes.data_as(C.POINTER(ULL)), t, records.ctypes.data_as(C.POINTER(ULL))) == -1
        want, moved = DR.slots_of(records, t)
        assert np.array_equal(slots, want) and (slots != EMPTY).sum() == 1 << t and max(moved) >= 2
        for j in (0, 1, 3, 5, (1 << t) - 1):
            assert plan.plan_dlog_home(ULL(int(records[j, 0])), t) == DR.home(records[j, 0], t) < 2 << t and plan.plan_dlog_tag(ULL(int(records[j, 0]))) == DR.tag(records[j, 0])
            assert plan.plan_dlog_find(slots.ctypes.data_as(C.POINTER(ULL)), t, records.ctypes.data_as(C.POINTER(ULL)), records[j].ctypes.data_as(C.POINTER(ULL))) == j
        absent = records[2].copy()
        absent[3] ^= np.uint64(1)                                                       # the same low word, another record: not found
        assert plan.plan_dlog_find(slots.ctypes.data_as(C.POINTER(ULL)), t, records.ctypes.data_as(C.POINTER(ULL)), absent.ctypes.data_as(C.POINTER(ULL))) == -1


def test_a_record_that_occurs_twice_is_refused(plan):
    rng = np.random.default_rng(DR.SEED + 41)
    records = rng.integers(0, 1 << 63, size=(64, 4), dtype=np.uint64)
    records[41] = records[7]
    slots = np.zeros(128, dtype=np.uint64)
    assert plan.plan_dlog_build_slots(slots.ctypes.data_as(C.POINTER(ULL)), 6, records.ctypes.data_as(C.POINTER(ULL))) == 41
    records[41, 3] ^= np.uint64(1 << 63)                                                # the parity bit alone tells them apart
    assert plan.plan_dlog_build_slots(slots.ctypes.data_as(C.POINTER(ULL)), 6, records.ctypes.data_as(C.POINTER(ULL))) == -1
