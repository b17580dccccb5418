"""CPU tier: the joint schedule zc_ed_lincomb_shared / zc_ris_lincomb_shared build from their scalar vector on the host
(dusk_zerocaf_amd/csrc/zc_shared_scalar.h: shared_lincomb_schedule), driven by g++ alone through tests/emul/
shared_lincomb_plan_emul.cpp.  Per term the steps must add up to k_eff (Edwards form) or (k_eff mod L) / 2 mod L (wire form) on
Python integers, with L from oracle/pymodel.py and the early-stop rule from tests/point_classes.  The sanitizer run is a
stand-alone program (tests/emul/shared_lincomb_plan_san.cpp) replaying a vector file as a child process: nothing sanitized is
loaded here."""
import ctypes as C
import os
import random
import struct

import numpy as np
import pytest

from oracle import pymodel as pm
from tests import emul_build as EB
from tests import point_classes as PC
from tests import shared_scalar_rows as S

M52 = (1 << 52) - 1
MAX_TERMS, MAX_STEPS = 8, 53
SEED = S.SEED + 0x11C


@pytest.fixture(scope="module")
def emul():
    so = EB.library("shared_lincomb_plan_emul.cpp")
    if so is None:
        pytest.skip("ROCm headers not present")
    lib = C.CDLL(so)
    lib.emul_shared_lincomb_plan_words.restype = C.c_int
    lib.emul_shared_lincomb_schedule_bytes.restype = C.c_int
    return lib


def value(words):
    return sum((int(w) & M52) << (52 * i) for i, w in enumerate(words))


def vectors():
    """[(what, [five words] * t)]: for t = 1..8 every edge scalar in every term position among random ones, the same edge scalar
    in every position, and 200 random vectors in all."""
    rng = random.Random(SEED)
    rnd = lambda: pm.limbs(rng.randrange(1 << rng.choice([252, 252, 252, 260, 128, 12])))
    out = []
    for t in range(1, MAX_TERMS + 1):
        for e, edge in enumerate(S.edge_scalars()):
            for j in range(t):
                out.append(("t=%d edge %d at %d" % (t, e, j), [list(edge) if i == j else rnd() for i in range(t)]))
            out.append(("t=%d edge %d everywhere" % (t, e), [list(edge) for _ in range(t)]))
        for r in range(25):
            out.append(("t=%d random %d" % (t, r), [pm.limbs(rng.randrange(1 << 252)) for _ in range(t)]))
    return out


def plan(lib, vec):
    """{ed, wire: (steps [(doublings, digit, term)], tail, terms, entries[8]), raw} for one scalar vector."""
    nw = lib.emul_shared_lincomb_plan_words()
    k = np.array(vec, dtype=np.uint64).reshape(-1)
    out = np.full(nw + 2, -7, dtype=np.int64)
    lib.emul_shared_lincomb_plan(C.c_void_p(k.ctypes.data), C.c_size_t(len(vec)), C.c_void_p(out[1:].ctypes.data))
    assert out[0] == -7 and out[-1] == -7 and [int(x) for x in k] == [int(x) for w in vec for x in w]
    o = [int(x) for x in out[1:-1]]
    res, at = {"raw": o}, 0
    for form in ("ed", "wire"):
        steps, tail, terms = o[at:at + 3]
        entries = o[at + 3:at + 3 + MAX_TERMS]
        body = o[at + 3 + MAX_TERMS:at + 3 + MAX_TERMS + 3 * MAX_STEPS * MAX_TERMS]
        assert 0 <= steps <= MAX_STEPS * MAX_TERMS and not any(body[3 * steps:])
        res[form] = ([tuple(body[3 * i:3 * i + 3]) for i in range(steps)], tail, terms, entries)
        at += nw // 2
    return res


def single(lib, words):
    out = np.zeros(2 * (2 + 2 * MAX_STEPS), dtype=np.int64)
    k = np.array(words, dtype=np.uint64)
    lib.emul_shared_single_plan(C.c_void_p(k.ctypes.data), C.c_void_p(out.ctypes.data))
    o, res = [int(x) for x in out], {}
    for f, form in enumerate(("ed", "wire")):
        at = f * (2 + 2 * MAX_STEPS)
        res[form] = ([(o[at + 2 + 2 * i], o[at + 3 + 2 * i]) for i in range(o[at])], o[at + 1])
    return res


def check(sched, want, what):
    """`want`: the integer of every term.  Positions are rebuilt from the doublings and the tail."""
    steps, tail, terms, entries = sched
    t = len(want)
    assert terms == t and len(steps) <= MAX_STEPS * t, what
    pos = tail + sum(r for r, _, _ in steps[1:])                    # of the first step: every later step lies r lower
    assert not steps or steps[0][0] == 0, what
    per = [[] for _ in range(t)]
    last = None
    for i, (r, d, j) in enumerate(steps):
        pos -= r if i else 0
        assert d % 2 == 1 and abs(d) <= 15 and 0 <= j < t and r >= 0, (what, i, r, d, j)
        if last is not None:
            assert (pos, -j) < (last[0], -last[1]) and (r == 0) == (pos == last[0]), (what, i)      # downwards; ties in term order
        last = (pos, j)
        per[j].append((pos, d))
    assert pos == tail if steps else tail == 0, what
    for j in range(t):
        assert sum(d << p for p, d in per[j]) == want[j], (what, j)
        ps = [p for p, _ in per[j]]
        assert all(a - b >= 5 for a, b in zip(ps, ps[1:])), (what, j)                               # within a term at least 5 apart
        assert entries[j] == (max([abs(d) for _, d in per[j]], default=0) + 1) // 2, (what, j)
        assert len(per[j]) <= MAX_STEPS and (not per[j] or per[j][0][1] > 0), (what, j)
    assert not any(entries[t:]), what


def test_every_vector_adds_up_per_term_in_both_forms(emul):
    vecs = vectors()
    assert len(vecs) >= 8 * 22 + 200 and sum("random" in w for w, _ in vecs) == 200
    ties = 0
    for what, vec in vecs:
        got = plan(emul, vec)
        eff = [PC.effective_scalar(value(w)) for w in vec]
        check(got["ed"], eff, (what, "ed"))
        inv2 = (pm.L + 1) // 2
        check(got["wire"], [(k % pm.L) * inv2 % pm.L for k in eff], (what, "wire"))
        ties += sum(1 for r, _, _ in got["ed"][0][1:] if r == 0)
    assert ties > 1000                                                                             # steps without doublings are common


def test_zero_vectors_equal_scalars_and_simple_coefficients(emul):
    for t in range(1, MAX_TERMS + 1):
        got = plan(emul, [[0] * 5] * t)
        assert got["ed"] == ([], 0, t, [0] * 8) and got["wire"] == ([], 0, t, [0] * 8)
        assert plan(emul, [pm.limbs(pm.L)] * t)["wire"] == ([], 0, t, [0] * 8)                       # L mod L = 0
    k = pm.limbs(0x1234567890ABCDEF1234567890ABCDEF)
    steps, tail, _, entries = plan(emul, [k, k])["ed"]
    assert len(steps) % 2 == 0 and entries[0] == entries[1]
    for a, b in zip(steps[0::2], steps[1::2]):
        assert b[0] == 0 and a[1] == b[1] and (a[2], b[2]) == (0, 1)                                # k_0 == k_1: pairs, no doublings between
    # (1, L - 1): ElGamal decryption with x = 1 -- the coefficient 1 needs one table record
    steps, tail, _, entries = plan(emul, [pm.limbs(1), pm.limbs(pm.L - 1)])["ed"]
    assert entries[0] == 1 and 1 <= entries[1] <= 8 and tail == 0 and [(d, j) for _, d, j in steps if j == 0] == [(1, 0)]
    assert plan(emul, [pm.limbs(1 << 200), pm.limbs(0), pm.limbs(3)])["ed"] == ([(0, 1, 0), (200, 3, 2)], 0, 3, [1, 0, 2, 0, 0, 0, 0, 0])
    assert plan(emul, [pm.limbs(0), pm.limbs(48)])["ed"] == ([(0, 3, 1)], 4, 2, [0, 2, 0, 0, 0, 0, 0, 0])


def test_one_term_is_the_single_scalar_schedule(emul):
    rng = random.Random(SEED + 1)
    for k in S.edge_scalars() + [pm.limbs(rng.randrange(1 << 252)) for _ in range(50)]:
        got, want = plan(emul, [k]), single(emul, k)
        for form in ("ed", "wire"):
            steps, tail, terms, _ = got[form]
            assert ([(r, d) for r, d, _ in steps], tail) == want[form] and terms == 1 and not any(j for _, _, j in steps)


def test_the_struct_is_a_fixed_size_pod_well_under_the_kernel_arguments(emul):
    assert emul.emul_shared_lincomb_schedule_bytes() == 4 * (3 + MAX_TERMS + MAX_STEPS * MAX_TERMS) == 1740
    assert emul.emul_shared_lincomb_plan_words() == 2 * (3 + MAX_TERMS + 3 * MAX_STEPS * MAX_TERMS)
    text = open(os.path.join(EB.CSRC, "zc_shared_scalar.h")).read()
    assert "static_assert(sizeof(shared_lincomb_schedule)" in text and "#include <hip" not in text


def test_the_densest_vector_fills_the_step_bound(emul):
    v = sum(1 << (5 * i) for i in range(52))
    steps, tail, _, entries = plan(emul, [pm.limbs(v)] * 8)["ed"]
    assert len(steps) == 52 * 8 and tail == 0 and entries == [1] * 8
    w = pm.limbs(sum(17 << (5 * i) for i in range(52)) % (1 << 260))
    got = plan(emul, [w] * 8)
    check(got["ed"], [PC.effective_scalar(value(w))] * 8, "carries")
    assert len(got["ed"][0]) <= MAX_STEPS * 8


def test_stand_alone_program_under_asan_and_ubsan(tmp_path, emul):
    """tests/emul/shared_lincomb_plan_san.cpp with -fsanitize=address,undefined -fno-sanitize-recover=all on every fourth vector of
    the list; its exit status is the verdict."""
    exe = EB.sanitizer_program("shared_lincomb_plan_san.cpp", tmp_path)
    vecs = vectors()[::4]
    assert {len(v) for _, v in vecs} == set(range(1, 9))
    nw = emul.emul_shared_lincomb_plan_words()
    parts = []
    for _, vec in vecs:
        flat = [x for w in vec for x in w]
        parts.append(struct.pack("<q%dQ" % len(flat), len(vec), *flat) + struct.pack("<%dq" % nw, *plan(emul, vec)["raw"]))
    blob = b"".join(parts) + struct.pack("<q", 0)
    EB.assert_clean(EB.run_vectors(exe, blob, tmp_path, "vectors.bin"), "%d cases match" % len(vecs))
    # the verdict is a real one: one expected word changed and the program says so
    bad = bytearray(blob)
    bad[len(parts[0]) + 8 * (1 + 5 * len(vecs[1][1]))] ^= 1                     # the step count of the second vector's first schedule
    EB.assert_caught(EB.run_vectors(exe, bad, tmp_path, "wrong.bin"), "case 1: word 0")
