"""CPU tier: the device functions behind the bounded discrete logs (zc_dlog.hip.h: dlog_setup, dlog_build_run, dlog_start,
dlog_search; zc_dlog_plan.h: slot array and slices), built for the host by tests/emul/dlog_emul.cpp in the plain and the
bounds-asserting (-DZC_CHECK_BOUNDS) build.  A point's record against the affine values of the oracle's ed_to_affine; table
build, sliced search and both forms against the planted truth of tests/dlog_rows.py at 2^4 and 2^6 records; the search cut at
arbitrary giant steps.  The sanitizer run is a stand-alone program (tests/emul/dlog_san.cpp) replaying a vector file as a child
process: nothing sanitized is loaded here."""
import ctypes as C
import struct

import numpy as np
import pytest

from tests import dlog_rows as DR
from tests import emul_build as EB

PC, GR = DR.PC, DR.GR


@pytest.fixture(scope="module", params=["plain", "checked"])
def emul(request):
    so = EB.library("dlog_emul.cpp", checked=request.param == "checked")
    if so is None:
        pytest.skip("ROCm headers not present")
    return DR.Emul(C.CDLL(so))


@pytest.fixture(scope="module")
def built(emul, oracle):
    """(generator, bits, coset4) -> Table, each built once per library."""
    out = {}
    for name in DR.GENERATORS:
        for t in DR.EMUL_BITS:
            for c in (0, 1):
                verdict, out[name, t, c] = emul.create(DR.generator(oracle, name), t, c)
                assert verdict == 0, (name, t, c)
    return out


def test_the_rows_are_what_the_issue_asks_for(emul, oracle):
    c = emul.constants()
    assert c == {k: DR.plan_constants()[k] for k in c}                                  # the text of zc_dlog_plan.h, read by the rows, is what was compiled
    Ck, S = c["chunk"], c["steps_per_launch"]
    for t in DR.EMUL_BITS + (9,):
        T, bound = 1 << t, DR.bound_for(t)
        hit, miss = DR.found_values(t), DR.missed_values(t)
        want = [0, 1, T - 1, T, T + 1, (Ck - 1) * T + T - 1, Ck * T, Ck * T + 1, S * T - 1, S * T, S * T + 1, bound - 1]
        assert set(want) <= set(hit) and max(hit) == bound - 1 and bound % T and bound > S * T + 1
        assert miss[:2] == [bound, bound + 1] and (bound - 1) >> t == bound >> t == (bound + 1) >> t       # at and above the bound, in the last giant step
        assert DR.pm.L - 1 in miss and (t > 6 or set(range(T)) <= set(hit))
    R = DR.ed_rows(oracle, "mixed", 4, 1)
    half = len(R["points"]) // 2
    assert not np.array_equal(R["points"][:half], R["points"][half:]) and oracle.mt(oracle.ed_eq, R["points"][:half].copy(), R["points"][half:].copy()).all()
    assert np.array_equal(R["m"][:half], R["m"][half:]) and 0 < R["found"].sum() < len(R["found"])
    assert DR.generator(oracle, "multiple")[10:15].tolist() != DR.pm.limbs(1)
    assert PC.order_in_e8(oracle, PC.times_L(oracle, DR.rows_of(DR.generator(oracle, "mixed")))) == 8


def test_record_of_a_point_is_the_oracles_affine_y_and_the_parity_of_x(emul, oracle):
    cl = PC.classes(oracle, 12, DR.SEED + 30)
    pts = np.concatenate([cl[k] for k in ("subgroup", "torsion", "order_2L", "order_8L", "decoded", "scaled")])
    want = DR.record_of(oracle, pts)
    got = np.stack([emul.record(p) for p in pts])
    assert np.array_equal(got, want)
    assert {int(r[3] >> np.uint64(63)) for r in want} == {0, 1}
    assert got[12].tolist() == [1, 0, 0, 0]                                             # the identity: y = 1, x = 0
    scaled = PC.scale(oracle, pts, DR.SEED + 31)
    assert np.array_equal(np.stack([emul.record(p) for p in scaled]), want)             # whatever the representative
    assert len({r.tobytes() for r in got}) == len({bytes(b) for b in oracle.mt(oracle.ed_compress, np.ascontiguousarray(pts))[0]})      # as injective as ed_compress


@pytest.mark.parametrize("coset4", [0, 1])
@pytest.mark.parametrize("t", DR.EMUL_BITS)
@pytest.mark.parametrize("name", DR.GENERATORS)
def test_table_is_the_records_of_the_multiples_filed_in_index_order(emul, built, oracle, name, t, coset4):
    tb = built[name, t, coset4]
    want = DR.table_records(oracle, name, t, coset4)
    assert np.array_equal(tb.records.reshape(-1, 4), want) and len({r.tobytes() for r in want}) == 1 << t
    slots, moved = DR.slots_of(want, t)
    assert np.array_equal(tb.slots, slots)
    # a generator in other coordinates and with another T builds the same table
    G = GR.with_true_t(oracle, DR.rows_of(DR.generator(oracle, name)))
    verdict, again = emul.create(PC.scale(oracle, G, DR.SEED + 32)[0], t, coset4)
    assert verdict == 0 and np.array_equal(again.records, tb.records) and np.array_equal(again.slots, tb.slots) and np.array_equal(again.setup, tb.setup)


@pytest.mark.parametrize("coset4", [0, 1])
@pytest.mark.parametrize("t", DR.EMUL_BITS)
@pytest.mark.parametrize("name", DR.GENERATORS)
def test_ed_form_finds_the_planted_m_and_nothing_else(emul, built, oracle, name, t, coset4):
    R = DR.ed_rows(oracle, name, t, coset4)
    tb = built[name, t, coset4]
    m, found, ok = emul.search(tb, R["points"], R["bound"])
    bad = np.flatnonzero((m != R["m"]) | (found != R["found"]))
    assert len(bad) == 0, [(R["what"][i], int(m[i]), int(found[i])) for i in bad[:6]]
    assert ok.all()
    # ok = NULL, and a row's answer is its own
    m2, f2, _ = emul.search(tb, R["points"], R["bound"], want_ok=False)
    assert np.array_equal(m2, m) and np.array_equal(f2, found)
    for i in (0, 7, len(m) - 1):
        one = emul.search(tb, R["points"][i:i + 1], R["bound"])
        assert one[0][0] == m[i] and one[1][0] == found[i]
    # a larger bound finds the rows between the two as well, and the others as before
    big = R["bound"] + 5 * (1 << t) + 1
    m3, f3, _ = emul.search(tb, R["points"], big)
    hit = found == 1
    assert np.array_equal(m3[hit], m[hit]) and f3[hit].all()
    extra = [i for i, w in enumerate(R["what"]) if "not below the bound" in w and "m=%d " % (DR.pm.L - 1) not in w and int(w.split()[0][2:]) < big]
    assert len(extra) == 6 and all(f3[i] == 1 and m3[i] == int(R["what"][i].split()[0][2:]) for i in extra)


@pytest.mark.parametrize("t", DR.EMUL_BITS)
@pytest.mark.parametrize("name", DR.GENERATORS)
def test_search_cut_at_arbitrary_giant_steps_gives_the_same_answers(emul, built, oracle, name, t):
    c = emul.constants()
    S, Ck = c["steps_per_launch"], c["chunk"]
    R = DR.ed_rows(oracle, name, t, 1)
    last = (R["bound"] - 1 >> t) + 1
    for cuts in ([0, last], [0, Ck, last], [0, 3 * Ck, 17 * Ck + 1, S - Ck, S + 1, last], [0, S // 2, S, last]):
        m, found, _ = emul.search(built[name, t, 1], R["points"], R["bound"], cuts=cuts, want_ok=False)
        assert np.array_equal(m, R["m"]) and np.array_equal(found, R["found"]), cuts
    # a search that ends a chunk early (a launch walks whole chunks) misses exactly the rows of the giant steps it left out
    end = (last - 1) // Ck * Ck
    m, found, _ = emul.search(built[name, t, 1], R["points"], R["bound"], cuts=[0, end], want_ok=False)
    lost = [i for i in range(len(m)) if found[i] != R["found"][i]]
    assert lost == [i for i in range(len(m)) if R["found"][i] == 1 and int(R["m"][i]) >> t >= end] != []


@pytest.mark.parametrize("t", DR.EMUL_BITS)
@pytest.mark.parametrize("name", DR.WIRE_GENERATORS)
def test_wire_form_decodes_finds_and_flags(emul, built, oracle, name, t):
    W = DR.wire_rows(oracle, name, t)
    m, found, ok = emul.search(built[name, t, 1], W["enc"], W["bound"], wire=True)
    assert np.array_equal(m, W["m"]) and np.array_equal(found, W["found"]) and np.array_equal(ok, W["ok"])
    assert W["ok"].sum() < len(W["ok"]) and not W["enc"][np.flatnonzero(W["ok"])[-1]].any()         # undecodable rows, and the identity as 32 zero bytes
    # the encodings decode to other representatives than the planted points: the same answers from their limbs
    pts, dec = oracle.ris_decompress(np.ascontiguousarray(W["enc"]))
    good = dec == 1
    m2, f2, ok2 = emul.search(built[name, t, 1], np.ascontiguousarray(pts[good]), W["bound"])
    assert np.array_equal(m2, W["m"][good]) and np.array_equal(f2, W["found"][good]) and ok2.all()


def test_hostile_rows_poison_only_themselves_and_bad_generators_are_refused(emul, oracle):
    hostile = DR.hostile_points(oracle)
    assert oracle.ed_is_valid(hostile[:2]).tolist() == [0, 1]                            # Z = 0 passes the projective equation
    for flags in (0, 1):
        assert [emul.create(p, 4, flags)[0] for p in hostile[:2]] == [1, 1]
        assert [emul.create(p, 4, flags)[0] for p in PC.torsion(oracle)] == [2] * 8
    assert emul.create(oracle.ed_add(GR.basepoint(), PC.torsion(oracle)[2:3])[0], 4, 1)[0] == 0          # B + T4: 4 G_eff = 4 B
    _, tb = emul.create(DR.generator(oracle, "B"), 4, 0)
    good = DR.multiples(oracle, DR.generator(oracle, "B"), [3, 17, 40])
    rows = np.concatenate([good[:1], hostile[:1], good[1:2], hostile[1:2], hostile[2:3], good[2:]])
    m, found, ok = emul.search(tb, rows, 64)
    assert m.tolist() == [3, 0, 17, 0, 0, 40] and found.tolist() == [1, 0, 1, 0, 0, 1] and ok.tolist() == [1, 0, 1, 0, 0, 1]


def test_the_whole_tier_passes_as_the_mutant_test_runs_it(emul, oracle):
    assert DR.failures(emul.lib, oracle) == []


def test_stand_alone_program_under_asan_and_ubsan(tmp_path, oracle):
    """tests/emul/dlog_san.cpp with -fsanitize=address,undefined -fno-sanitize-recover=all: setup block, records, slots, rows and
    outputs in heap blocks of exactly their size; its exit status is the verdict."""
    exe = EB.sanitizer_program("dlog_san.cpp", tmp_path)
    parts, rows = [], 0
    R = DR.ed_rows(oracle, "mixed", 4, 0)
    pts = np.concatenate([R["points"][:40], DR.hostile_points(oracle)])
    want = [np.concatenate([R[k][:40].astype(np.uint64), np.zeros(3, dtype=np.uint64)]) for k in ("m", "found")] + [np.array([1] * 40 + [0] * 3, dtype=np.uint64)]
    parts.append(struct.pack("<5Q", 0, 4, 0, R["bound"], len(pts)) + DR.generator(oracle, "mixed").tobytes() + np.ascontiguousarray(pts).tobytes() + b"".join(w.tobytes() for w in want))
    rows += len(pts)
    W = DR.wire_rows(oracle, "multiple", 6)
    parts.append(struct.pack("<5Q", 1, 6, 1, W["bound"], len(W["enc"])) + DR.generator(oracle, "multiple").tobytes() + W["enc"].tobytes() +
                 b"".join(W[k].astype(np.uint64).tobytes() for k in ("m", "found", "ok")))
    rows += len(W["enc"])
    blob = b"".join(parts) + struct.pack("<Q", 2)
    EB.assert_clean(EB.run_vectors(exe, blob, tmp_path, "vectors.bin"), "2 records, %d rows match" % rows)
    bad = bytearray(blob)
    bad[-16] ^= 1                                                                       # the last row's expected ok
    EB.assert_caught(EB.run_vectors(exe, bad, tmp_path, "wrong.bin"), "record 1: row %d:" % (len(W["enc"]) - 1))
