"""CPU tier: what zc_ed_scalar_mul_shared / zc_ris_mul_shared do with their one scalar on the host (dusk_zerocaf_amd/csrc/
zc_shared_scalar.h), driven by g++ alone through tests/emul/shared_scalar_plan_emul.cpp: the effective scalar (the same value
as the device's scalar_effective, built for the host beside it, and as the reference's loop on Python integers), k' = (k_eff
mod L) / 2 mod L, and the width-5 signed sliding-window schedule of either.  The sanitizer run is a stand-alone program
(tests/emul/shared_scalar_plan_san.cpp) replaying a vector file as a child process: nothing sanitized is loaded here."""
import ctypes as C
import random
import struct

import numpy as np
import pytest

from oracle import pymodel as pm
from tests import emul_build as EB
from tests import point_classes as PC
from tests import vectors as V

M52 = (1 << 52) - 1
MAX_STEPS = 53
SEED = V.SEED + 0x5A4ED


def words_of(v):
    """Five 52-bit limbs of an integer below 2^260."""
    assert 0 <= v < 1 << 260
    return [(v >> (52 * i)) & M52 for i in range(5)]


def scalar_patterns():
    """[(name, five u64 words)]: the issue's list."""
    L, t = pm.L, 1 << 48
    named = [0, 1, 2, 3, 15, 16, 17, 31, 32, 33, L - 1, L, L + 1, 2 * L + 5, 1 << 249, (1 << 252) - 1, (1 << 256) - 1]
    pats = [("%d" % v if v < 64 else "edge %d" % i, words_of(v)) for i, v in enumerate(named)]
    # at or above 2^256, on both sides of the early-stop rule (low256 < 2^ctz(hi) stops early)
    for w in V.raw_scalar_edges():
        pats.append(("raw", [int(x) for x in w]))
    pats.append(("2^259 + 8: digits 256 apart", [8, 0, 0, 0, 8 * t]))
    # bits from 2^52 up in the words: outside the contract, masked
    rng = random.Random(SEED)
    for i in range(16):
        w = words_of(rng.randrange(1 << 260))
        pats.append(("high bits", [x | (rng.randrange(1, 1 << 12) << 52) for x in w]))
    pats.append(("all ones", [(1 << 64) - 1] * 5))
    for i in range(2000):
        bits = rng.choice([260, 260, 256, 253, 249, 128, 64, 12])
        pats.append(("random", words_of(rng.randrange(1 << bits))))
    return pats


@pytest.fixture(scope="module")
def emul():
    so = EB.library("shared_scalar_plan_emul.cpp")
    if so is None:
        pytest.skip("ROCm headers not present")
    lib = C.CDLL(so)
    lib.emul_shared_plan_words.restype = C.c_int
    return lib


def plan(lib, words):
    """{host, dev, half: integers; ed, wire: (steps [(doublings, digit)], tail)} for one scalar, plus the raw words."""
    nw = lib.emul_shared_plan_words()
    k = np.array(words, dtype=np.uint64)
    out = np.full(nw + 2, -7, dtype=np.int64)
    lib.emul_shared_plan(C.c_void_p(k.ctypes.data), C.c_void_p(out[1:].ctypes.data))
    assert out[0] == -7 and out[-1] == -7 and [int(x) for x in k] == [int(x) for x in words]
    o = [int(x) for x in out[1:-1]]
    val = lambda l: sum(x << (52 * i) for i, x in enumerate(l))
    res = {"host": val(o[0:5]), "dev": val(o[5:10]), "half": val(o[10:15]), "raw": o, "limbs": o[0:15]}
    at = 15
    for form in ("ed", "wire"):
        steps, tail = o[at], o[at + 1]
        body = o[at + 2:at + 2 + 2 * MAX_STEPS]
        assert 0 <= steps <= MAX_STEPS and not any(body[2 * steps:])
        res[form] = ([(body[2 * i], body[2 * i + 1]) for i in range(steps)], tail)
        at += 2 + 2 * MAX_STEPS
    return res


def schedule_value(steps, tail):
    """The integer a walk of the schedule multiplies by: r doublings, then the digit, from the top down."""
    acc = 0
    for r, d in steps:
        acc = (acc << r) + d
    return acc << tail


def check_schedule(steps, tail, value, what):
    assert schedule_value(steps, tail) == value, what
    assert len(steps) <= MAX_STEPS, what
    for i, (r, d) in enumerate(steps):
        assert d % 2 == 1 and abs(d) <= 15, (what, i, d)                       # odd (Python: -3 % 2 == 1), at most 15
        assert (r == 0) if i == 0 else (5 <= r <= 260), (what, i, r)            # non-zero digits at least 5 positions apart
    if not steps:
        assert tail == 0 and value == 0, what
    else:
        assert steps[0][1] > 0 and 0 <= tail <= 260, what                       # the top digit of a positive value is positive


def test_every_scalar_of_the_list(emul):
    pats = scalar_patterns()
    assert len(pats) > 2000
    early = late = 0
    for name, words in pats:
        got = plan(emul, words)
        masked = sum((w & M52) << (52 * i) for i, w in enumerate(words))
        want = PC.effective_scalar(masked)
        assert got["host"] == got["dev"] == want, (name, words)
        if masked >= 1 << 256:
            early += want != masked
            late += want == masked
        check_schedule(*got["ed"], want, (name, words, "ed"))
        assert got["half"] < pm.L and 2 * got["half"] % pm.L == want % pm.L, (name, words)
        check_schedule(*got["wire"], got["half"], (name, words, "wire"))
    assert early >= 5 and late >= 5                                              # both sides of the early-stop rule


def test_the_schedule_of_zero_has_no_steps_and_small_ones_are_what_they_should_be(emul):
    assert plan(emul, [0] * 5)["ed"] == ([], 0) and plan(emul, [0] * 5)["wire"] == ([], 0)
    assert plan(emul, words_of(pm.L))["wire"] == ([], 0)                         # L mod L = 0
    assert plan(emul, [1, 0, 0, 0, 0])["ed"] == ([(0, 1)], 0)
    assert plan(emul, [16, 0, 0, 0, 0])["ed"] == ([(0, 1)], 4)
    assert plan(emul, [17, 0, 0, 0, 0])["ed"] == ([(0, 1), (5, -15)], 0)          # 17 = 32 - 15
    assert plan(emul, [31, 0, 0, 0, 0])["ed"] == ([(0, 1), (5, -1)], 0)
    assert plan(emul, [33, 0, 0, 0, 0])["ed"] == ([(0, 1), (5, 1)], 0)
    assert plan(emul, [2, 0, 0, 0, 0])["wire"] == ([(0, 1)], 0)                   # k' = 1
    assert plan(emul, [1, 0, 0, 0, 0])["half"] == (pm.L + 1) // 2
    assert plan(emul, [8, 0, 0, 0, 8 << 48])["ed"] == ([(0, 1), (256, 1)], 3)     # more than 255 doublings in one step
    dense = plan(emul, words_of(int("1" * 52, 2) * sum(1 << (52 * i) for i in range(5))))
    assert len(dense["ed"][0]) <= MAX_STEPS


def test_the_worst_case_count_of_steps(emul):
    """The densest recoding has a non-zero digit every five positions: 0b00001 repeated needs ceil(260 / 5) = 52 digits, and a
    carry out of the top can add one."""
    v = sum(1 << (5 * i) for i in range(52))
    steps, tail = plan(emul, words_of(v))["ed"]
    assert len(steps) == 52 and tail == 0
    v = sum(17 << (5 * i) for i in range(52)) % (1 << 260)                       # every window 10001: all digits negative, carries all the way
    got = plan(emul, words_of(v))
    check_schedule(*got["ed"], got["host"], "carries")
    assert len(got["ed"][0]) <= MAX_STEPS


def test_stand_alone_program_under_asan_and_ubsan(tmp_path, emul):
    """tests/emul/shared_scalar_plan_san.cpp with -fsanitize=address,undefined -fno-sanitize-recover=all on the whole list; its
    exit status is the verdict."""
    exe = EB.sanitizer_program("shared_scalar_plan_san.cpp", tmp_path)
    pats = scalar_patterns()
    blob = b""
    for name, words in pats:
        blob += struct.pack("<q5Q", 1, *words) + struct.pack("<%dq" % emul.emul_shared_plan_words(), *plan(emul, words)["raw"])
    blob += struct.pack("<q", 0)
    EB.assert_clean(EB.run_vectors(exe, blob, tmp_path, "vectors.bin"), "%d cases match" % len(pats))
    # the verdict is a real one: one expected word changed and the program says so
    bad = bytearray(blob)
    rec = 8 * (1 + 5 + emul.emul_shared_plan_words())
    bad[3 * rec + 8 * 6 + 8 * 15] ^= 1                                           # the step count of the fourth scalar's first schedule
    EB.assert_caught(EB.run_vectors(exe, bad, tmp_path, "wrong.bin"), "case 3: word 15")
