"""CPU tier: the host launch choices of the row-wise entry points (dusk_zerocaf_amd/csrc/zc_launch_plan.h) against a recorded table.

tests/emul/launch_plan_emul.cpp includes that header alone -- plain g++, no HIP -- and answers one launch decision per call:
the rows of a host chunk, the staged or the per-lane form of an element-wise or point op, the form and grid of a strict scalar
multiplication (with the permutation it asks for and its bytes), the form of an op with shared inversions, the geometry of the
windowed core's table ring, the lincombs' workgroup, the SHA-512 reader.  tests/golden/launch_plan_table.json holds the expected
fields over a grid that puts n - 1, n and n + 1 on every point where a rule branches, for every knob setting that changes the
branch (grid() below).

How the committed table was made: NOT from this header.  The constants, `if` ladders and predicates that zerocaf_hip.hip held
before the header existed (commit 835dcea: host_chunk_elems, the `staged` predicates of binop and unop with staged_min,
balance_index's size test, scalar_mul_on_device with strict_kernel_for and the small-shard MSM's direct use of it, inv_chunk
and launch_shared_inversions, ring_units_per_xcd and fast_ring's slot arithmetic, the block rule of the two lincombs, the
`words` test of hash_rows_call) were lifted verbatim into a throwaway program with the driver's C interface, and that program
wrote the table; the header must reproduce it.  After an intentional change of a launch rule,
`python -m tests.test_launch_plan_emul` rewrites the table from the current header -- review the diff of the table like code.

tests/entry_table.py mirrors four of the thresholds as literals (it is imported where nothing is compiled), and the GPU tier
picks its batch sizes from them; test_entry_table_mirrors_sit_on_the_header_boundaries pins them to the header's behaviour.
The sanitizer run is a stand-alone program (tests/emul/launch_plan_san.cpp) replaying a vector file as a child process: nothing
sanitized is loaded here."""
import ctypes as C
import json
import os
import struct

import pytest

from tests import emul_build as EB
from tests import entry_table as T
from tests import kill_vectors as KV
from tests.emul_build import CSRC, HERE

TABLE = os.path.join(HERE, "golden", "launch_plan_table.json")
HEADER = os.path.join(CSRC, "zc_launch_plan.h")

HOST_CHUNK, ELEMENTWISE, STRICT, INVERSION, RING, LINCOMB, HASH = range(7)
KINDS = {
    HOST_CHUNK: {"name": "host_chunk_elems", "args": ["cnt", "heavy", "forced"], "fields": ["chunk"]},
    ELEMENTWISE: {"name": "elementwise_form", "args": ["cnt", "limbs_per_row", "arrays", "has_staged", "point_threshold", "test_stream_min", "all_aligned16"],
                  "fields": ["form", "block"]},
    STRICT: {"name": "strict_form", "args": ["cnt", "sched_block", "sched_unified", "permutation_can_be_had", "cus", "quad_ok"],
             "fields": ["wants_permutation", "balance_bytes", "form", "grid"]},
    INVERSION: {"name": "inversion_form", "args": ["cnt", "in_place", "inv_chunk_knob", "cus"], "fields": ["form", "c", "lanes"]},
    RING: {"name": "ring_plan", "args": ["slot_units", "ring_slots_knob"], "fields": ["units_per_xcd", "slots", "max_launch", "table_bytes"]},
    LINCOMB: {"name": "lincomb_launch", "args": ["slots_used"], "fields": ["block", "lds_bytes"]},
    HASH: {"name": "hash_reader_words", "args": ["prefix_len", "force_bytes", "nparts", "part_len[nparts]", "ptr_mod8[nparts]"], "fields": ["words"]},
}
# zc::LaunchForm, in the header's order (test_form_names_are_the_headers)
FORMS = list(KV.LAUNCH_FORMS)
PER_LANE, STAGED, QUAD, SMALL, BLOCK, PW, PW_UNIFIED, INV_PER_ELEMENT, INV_CHUNKED, INV_LONE = range(10)

R = 1 << 17                                   # CHUNK_ROUND, PW_MIN_ELEMS
LANES = 1 << 16                               # INV_LANES_TARGET; 256 CUs x 256 lanes


def around(xs):
    return list(dict.fromkeys(y for x in xs for y in (x - 1, x, x + 1)))


def grid():
    """[kind, [arguments]] -- a few hundred cases; every threshold of the rules has its n - 1, n, n + 1."""
    rows = []
    # ---- host chunks: light batches stay whole; heavy ones: 2^17 rows from 2 x 2^17 on, from 4 x 2^17 on an eighth rounded up to
    # 2^17 but at least 2 x 2^17 (the rounding bites at 2^22 + 8, the floor lets go at 16 x 2^17 + 8); every chunk a multiple of 1024
    sizes = [1, 1023, 1024, 1025] + around([2 * R, 4 * R, 16 * R]) + [16 * R + 7, 16 * R + 8, (1 << 22) + 7, (1 << 22) + 8, (1 << 22) + 9, 1 << 26, (1 << 26) + 1]
    for heavy in (0, 1):
        rows += [[HOST_CHUNK, [n, heavy, 0]] for n in sizes]
        rows += [[HOST_CHUNK, [n, heavy, forced]] for forced in (1, 3, 4096) for n in (1, 4097, 3 * R + 5, 1 << 22)]
    rows += [[HOST_CHUNK, [n, 1, 1 << 20]] for n in [5000] + around([1 << 22]) + [1 << 33, (1 << 33) + 1]]      # MAX_CHUNKS binds from 2^22 + 1 on
    # ---- element-wise ops, 40-byte rows: three arrays cross STREAM_BYTES at 2 236 962 / 2 236 963 rows, two at 3 355 443 / 3 355 444
    for arrays, last in ((3, 2236962), (2, 3355443)):
        for aligned in (1, 0):
            for has_staged in (1, 0):
                rows += [[ELEMENTWISE, [n, 5, arrays, has_staged, 0, 0, aligned]] for n in (last - 1, last, last + 1, last + 2)]
                rows += [[ELEMENTWISE, [n, 5, arrays, has_staged, 0, 1, aligned]] for n in (1, 300)]              # ZC_TEST_STREAM_MIN_BYTES=1
        rows += [[ELEMENTWISE, [n, 5, arrays, 1, 0, 12000, 1]] for n in around([12000 // (40 * arrays)])]         # ... = 12000: 100 / 101, 150 / 151
    # ---- point ops, 160-byte rows: above 2^12 points for two and for three arrays, and the test knob does not move that
    for arrays in (3, 2):
        for aligned in (1, 0):
            for has_staged in (1, 0):
                for stream_min in (0, 1):
                    rows += [[ELEMENTWISE, [n, 20, arrays, has_staged, 1, stream_min, aligned]] for n in (1, 4095, 4096, 4097, 4098)]
    rows += [[ELEMENTWISE, [1 << 24, 15, arrays, 0, 0, 0, 1]] for arrays in (3, 2)]                              # the 120-byte rows have no staged kernel
    # ---- strict scalar multiplication
    sizes = [1, 2] + around([1 << 14, 1 << 16]) + [R - 2, R - 1, R, R + 1] + around([1 << 32])
    for sched_block, sched_unified in ((0, 0), (1, 0), (0, 1)):
        for can in (1, 0):
            rows += [[STRICT, [n, sched_block, sched_unified, can, 256, 1]] for n in sizes]
    rows += [[STRICT, [n, 0, u, 1, 64, 1]] for u in (0, 1) for n in (R - 1, R)]                                   # the persistent grid follows the CU count
    rows += [[STRICT, [n, 0, 0, 1, 256, 0]] for n in (1, 2, 255, 256, 257, 4095)]                                 # the products of a small zc_msm shard: never four lanes per row
    # ---- shared inversions: c = cnt / 2^16, so c = 2 first at 2^17 and the cap of 32 from 2^21 on; the lone form up to 256 lanes per CU
    for cus in (256, 304):
        for in_place in (0, 1):
            rows += [[INVERSION, [n, in_place, 0, cus]] for n in [1, 300] + around([1 << 17, 3 * LANES, 1 << 21, (1 << 21) + LANES, 2 * 304 * 256])]
    for knob in (1, 2, 7, 64):
        for in_place in (0, 1):
            rows += [[INVERSION, [n, in_place, knob, 256]] for n in [300, 301] + around([knob * LANES])]
    rows += [[INVERSION, [n, 0, 7, 304]] for n in around([7 * 304 * 256])]
    # ---- the table ring, the lincombs' workgroup
    rows += [[RING, [units, knob]] for units in range(1, 9) for knob in (0, 1, 7, 512)]
    rows += [[LINCOMB, [slots]] for slots in range(1, 9)]
    # ---- SHA-512 reader: words, then each condition flipped alone
    rows += [[HASH, a] for a in ([8, 0, 2, 32, 64, 0, 0], [7, 0, 2, 32, 64, 0, 0], [8, 1, 2, 32, 64, 0, 0], [8, 0, 2, 33, 64, 0, 0], [8, 0, 2, 32, 63, 0, 0],
                                 [8, 0, 2, 32, 64, 4, 0], [8, 0, 2, 32, 64, 0, 1], [0, 0, 1, 8, 0], [0, 0, 1, 1, 0], [0, 0, 1, 8, 7], [0, 1, 1, 8, 0], [4, 0, 1, 8, 0],
                                 [256, 0, 4, 8, 16, 24, 32, 0, 0, 0, 0], [256, 0, 4, 8, 16, 24, 36, 0, 0, 0, 0], [256, 0, 4, 8, 16, 24, 32, 0, 0, 0, 2])]
    return rows


def build_emul():
    so = EB.library("launch_plan_emul.cpp", flags=EB.STRICT)
    if so is None:
        pytest.skip("ROCm headers not present")
    return load(so)


def load(so):
    lib = C.CDLL(so)
    lib.emul_launch_plan.argtypes = [C.c_int, C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_int64)]
    return lib


def run_case(lib, case):
    kind, args = case
    out = (C.c_int64 * 8)()
    n = lib.emul_launch_plan(kind, (C.c_int64 * len(args))(*args), len(args), out)
    assert n == len(KINDS[kind]["fields"]), (case, n)
    return list(out[:n])


@pytest.fixture(scope="module")
def emul():
    return build_emul()


@pytest.fixture(scope="module")
def table():
    return json.load(open(TABLE))


def test_table_is_the_grid(table):
    assert table["kinds"] == {str(k): v for k, v in KINDS.items()} and table["forms"] == FORMS
    assert [r[:2] for r in table["rows"]] == grid()
    assert 300 <= len(table["rows"]) <= 800 and os.path.getsize(TABLE) <= os.path.getsize(os.path.join(HERE, "golden", "msm_plan_table.json"))


def test_form_names_are_the_headers():
    """FORMS is zc::LaunchForm: the enumerators in the header's order, closed by LAUNCH_FORMS."""
    import re
    body = re.search(r"enum LaunchForm \{(.*?)\};", open(HEADER).read(), re.S).group(1)
    names = re.findall(r"^\s*(FORM_[A-Z_]+|LAUNCH_FORMS)\b", body, re.M)
    assert names == ["FORM_" + f.upper() for f in FORMS] + ["LAUNCH_FORMS"]


def test_every_field_matches_the_recorded_table(emul, table):
    bad = []
    for kind, args, want in table["rows"]:
        got = run_case(emul, [kind, args])
        if got != want:
            bad.append((KINDS[kind]["name"], args, {f: (w, g) for f, w, g in zip(KINDS[kind]["fields"], want, got) if w != g}))
    assert not bad, "%d of %d cases differ (field: (recorded, header)), first: %r" % (len(bad), len(table["rows"]), bad[:3])


def test_table_covers_the_branches(table):
    """The grid is only worth its rows if the recorded outcomes really differ where the rules branch."""
    got = {(kind, tuple(args)): out for kind, args, out in table["rows"]}
    at = lambda kind, *args: got[(kind, args)]
    forms = lambda kind, i: {out[i] for (k, _), out in got.items() if k == kind}
    assert forms(ELEMENTWISE, 0) == {PER_LANE, STAGED} and forms(STRICT, 2) == {QUAD, SMALL, BLOCK, PW, PW_UNIFIED}
    assert forms(INVERSION, 0) == {INV_PER_ELEMENT, INV_CHUNKED, INV_LONE} and forms(HASH, 0) == {0, 1}
    assert sorted(forms(STRICT, 2) | forms(ELEMENTWISE, 0) | forms(INVERSION, 0)) == list(range(len(FORMS)))
    # host chunks: whole, 2^17, an eighth (floor, rounding), the forced counts, the chunk limit
    chunk = lambda n, heavy=1, forced=0: at(HOST_CHUNK, n, heavy, forced)[0]
    assert [chunk(n) for n in (2 * R - 1, 2 * R, 4 * R - 1, 4 * R)] == [2 * R, R, R, 2 * R] and chunk(4 * R, heavy=0) == 4 * R
    assert [chunk(n) for n in (16 * R + 7, 16 * R + 8, (1 << 22) + 7, (1 << 22) + 8)] == [2 * R, 3 * R, 4 * R, 5 * R]
    assert [chunk(3 * R + 5, forced=f) for f in (1, 3, 4096)] == [3 * R + 1024, R + 1024, 1024] and chunk(1, heavy=0) == 1024
    assert [chunk(n, forced=1 << 20) for n in (1 << 22, (1 << 22) + 1)] == [1024, 1025]
    # the staged forms: both sides of STREAM_BYTES and of 2^12 points, alignment, a staged kernel at all, the test knob
    for arrays, last in ((3, 2236962), (2, 3355443)):
        assert [at(ELEMENTWISE, n, 5, arrays, 1, 0, 0, 1)[0] for n in (last, last + 1)] == [PER_LANE, STAGED]
        assert at(ELEMENTWISE, last + 1, 5, arrays, 1, 0, 0, 0)[0] == PER_LANE and at(ELEMENTWISE, last + 1, 5, arrays, 0, 0, 0, 1)[0] == PER_LANE
        assert at(ELEMENTWISE, 1, 5, arrays, 1, 0, 1, 1)[0] == STAGED and at(ELEMENTWISE, 1, 5, arrays, 1, 0, 1, 0)[0] == PER_LANE
        assert [at(ELEMENTWISE, n, 20, arrays, 1, 1, s, 1)[0] for s in (0, 1) for n in (4096, 4097)] == [PER_LANE, STAGED] * 2
        assert at(ELEMENTWISE, 4097, 20, arrays, 1, 1, 0, 0)[0] == PER_LANE and at(ELEMENTWISE, 4097, 20, arrays, 0, 1, 0, 1)[0] == PER_LANE
    assert [at(ELEMENTWISE, n, 5, 3, 1, 0, 12000, 1)[0] for n in (100, 101)] == [PER_LANE, STAGED]
    assert [at(ELEMENTWISE, n, 5, 2, 1, 0, 12000, 1)[0] for n in (150, 151)] == [PER_LANE, STAGED]
    # strict: the four size thresholds, the three schedules, the fall-back without the permutation, 32-bit row indices
    strict = lambda n, b=0, u=0, can=1, cus=256, quad=1: at(STRICT, n, b, u, can, cus, quad)
    assert [strict(n)[2] for n in (1 << 14, (1 << 14) + 1, 1 << 16, (1 << 16) + 1, R - 1, R)] == [QUAD, SMALL, SMALL, BLOCK, BLOCK, PW]
    assert [strict(n)[3] for n in (1, 1 << 14, (1 << 14) + 1, (1 << 16) + 1, R)] == [1, 256, 65, 257, 768] and strict(R, cus=64)[3] == 192
    assert strict(R, u=1)[2] == PW_UNIFIED and strict(R, b=1)[:3] == [0, 0, BLOCK] and strict(R - 1, u=1)[2] == BLOCK
    assert strict(R)[:2] == [1, (1024 + 64 + R) * 4] and strict(R, can=0) == [1, (1024 + 64 + R) * 4, BLOCK, 512] and strict(R - 1)[:2] == [0, 0]
    assert strict((1 << 32) - 1)[::2] == [1, PW] and strict(1 << 32) == [0, 0, BLOCK, 1 << 24]
    assert [strict(n, quad=0)[2:] for n in (1, 4095)] == [[SMALL, 1], [SMALL, 16]] and strict(1)[2:] == [QUAD, 1]
    # inversions: c = 2 first at 2^17, the cap, the lone form's lane limit for two CU counts, the knob, in place
    inv = lambda n, in_place=0, knob=0, cus=256: at(INVERSION, n, in_place, knob, cus)
    assert [inv(n) for n in (R - 1, R, R + 1)] == [[INV_PER_ELEMENT, 1, R - 1], [INV_LONE, 2, LANES], [INV_CHUNKED, 2, LANES + 1]]
    assert inv(R, in_place=1) == [INV_PER_ELEMENT, 2, R] and [inv(n)[1] for n in ((1 << 21) - 1, 1 << 21, (1 << 21) + LANES)] == [31, 32, 32]
    assert [inv(n, cus=304)[0] for n in (2 * 304 * 256, 2 * 304 * 256 + 1)] == [INV_LONE, INV_CHUNKED] and inv(2 * 304 * 256)[0] == INV_CHUNKED
    assert [inv(n, knob=7, cus=304)[0] for n in (7 * 304 * 256, 7 * 304 * 256 + 1)] == [INV_LONE, INV_CHUNKED]
    assert inv(301, knob=1) == [INV_PER_ELEMENT, 1, 301] and inv(301, knob=2) == [INV_LONE, 2, 151] and inv(300, knob=7) == [INV_LONE, 7, 43]
    assert [inv(n, knob=64) for n in (64 * LANES, 64 * LANES + 1)] == [[INV_LONE, 64, LANES], [INV_CHUNKED, 64, LANES + 1]]
    # the ring: slots per XCD by slot size, the knob, rows per launch (2^24 per slot, at most 2^31), the table area
    assert [at(RING, u, 0)[1] for u in range(1, 9)] == [512, 512, 512, 512, 409, 341, 292, 256]
    assert [at(RING, u, 0)[0] for u in range(1, 9)] == [512, 1024, 1536, 2048, 2048, 2048, 2048, 2048]
    assert [at(RING, 8, k)[1:3] for k in (1, 7, 512)] == [[1, 1 << 24], [7, 7 << 24], [256, 1 << 31]] and at(RING, 1, 0)[2:] == [1 << 31, 256 << 20]
    assert at(RING, 8, 0)[3] == 1 << 30
    assert [at(LINCOMB, s) for s in (1, 4, 5, 8)] == [[256, 36 * 256], [256, 36 * 4 * 256], [128, 36 * 5 * 128], [128, 36 * 8 * 128]]
    assert [out[0] for (k, _), out in got.items() if k == HASH] == [1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0]


def test_entry_table_mirrors_sit_on_the_header_boundaries(emul):
    """tests/entry_table.py's literals choose the GPU tier's batch sizes: the header gives one form AT each constant and the
    next form one row later (asked of the header itself, not read from its text)."""
    point = lambda n, arrays: run_case(emul, [ELEMENTWISE, [n, 20, arrays, 1, 1, 0, 1]])[0]
    strict = lambda n: run_case(emul, [STRICT, [n, 0, 0, 1, 256, 1]])[2]
    for arrays in (2, 3):
        assert [point(T.ED_STAGED_MIN_POINTS + d, arrays) for d in (0, 1)] == [PER_LANE, STAGED]
    assert [strict(T.QUAD_LAUNCH_ELEMS + d) for d in (0, 1)] == [QUAD, SMALL]
    assert [strict(T.STRICT_SMALL_MAX_ELEMS + d) for d in (0, 1)] == [SMALL, BLOCK]
    assert [strict(T.PW_MIN_ELEMS + d) for d in (-1, 0)] == [BLOCK, PW]


# ------------------------------------------------------------------ the stand-alone sanitizer run
def vector_file(rows):
    """Records of little-endian 64-bit words: kind + 1 (0: end), number of arguments, number of fields, the arguments, the fields."""
    words = []
    for kind, args, want in rows:
        words += [kind + 1, len(args), len(want)] + list(args) + list(want)
    return struct.pack("<%dq" % (len(words) + 1), *(words + [0]))


def test_stand_alone_program_under_asan_and_ubsan(tmp_path, table):
    """tests/emul/launch_plan_san.cpp with -fsanitize=address,undefined -fno-sanitize-recover=all on the whole table (the shifts,
    casts and products at 2^32 and 2^33 rows among it); its exit status is the verdict."""
    exe = EB.sanitizer_program("launch_plan_san.cpp", tmp_path, flags=EB.STRICT)
    rows = table["rows"]
    EB.assert_clean(EB.run_vectors(exe, vector_file(rows), tmp_path, "vectors.bin"), "%d cases match" % len(rows))
    # the verdict is a real one: one expected field changed and the program says so
    i = next(j for j, r in enumerate(rows) if r[0] == STRICT)
    bad = [list(r) for r in rows]
    bad[i] = [rows[i][0], rows[i][1], rows[i][2][:3] + [rows[i][2][3] + 1]]
    EB.assert_caught(EB.run_vectors(exe, vector_file(bad), tmp_path, "wrong.bin"), "case %d (kind %d): field 3" % (i, STRICT))


def write_table(lib, path):
    rows = [case + [run_case(lib, case)] for case in grid()]
    with open(path, "w") as f:
        f.write('{"kinds": %s,\n "forms": %s,\n "case": ["kind", "arguments", "fields"],\n "rows": [\n' % (json.dumps({str(k): v for k, v in KINDS.items()}), json.dumps(FORMS)))
        f.write(",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in rows))
        f.write("\n ]}\n")
    return len(rows)


if __name__ == "__main__":
    print("%d rows -> %s" % (write_table(build_emul(), TABLE), TABLE))
