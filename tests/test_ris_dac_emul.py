"""CPU tier: the device functions behind zc_ris_double_and_compress (zc_ris_batch.hip.h: ris_double_compress_row,
ris_double_compress_chunk), built for the host by tests/emul/ris_dac_emul.cpp in the plain and the bounds-asserting
(-DZC_CHECK_BOUNDS) build.  Every row is compared with the C oracle's ris_compress(ed_double(P)); the formula itself is checked
on Python integers against oracle/pymodel.py, so both oracles are on record.  The sanitizer run is a stand-alone program
(tests/emul/ris_dac_san.cpp) replaying a vector file as a child process: nothing sanitized is loaded here."""
import ctypes as C
import random
import struct

import numpy as np
import pytest

from oracle import pymodel as pm
from tests import emul_build as EB
from tests import hostile_rows as H
from tests import point_classes as PC
from tests import vectors as V

CHUNKS = [1, 2, 3, 16, 64]
SEED = V.SEED + 0xDAC0


@pytest.fixture(scope="module", params=["plain", "checked"])
def emul(request):
    checked = request.param == "checked"
    so = EB.library("ris_dac_emul.cpp", checked=checked)
    if so is None:
        pytest.skip("ROCm headers not present")
    lib = C.CDLL(so)
    lib.checked = checked
    return lib


def dac(lib, rows, c=0, ilp=0):
    """c = 0: one row per lane (k_ris_double_compress); else the shared inversions at c rows per lane.  The output is framed:
    nothing outside the n rows may change."""
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    n = len(rows)
    buf = np.full(32 * (n + 2), 0xA5, dtype=np.uint8)
    before = rows.copy()
    out = buf[32:32 * (n + 1)]
    if c == 0:
        lib.emul_ris_dac_rows(C.c_void_p(rows.ctypes.data), C.c_void_p(out.ctypes.data), C.c_size_t(n))
    else:
        lib.emul_ris_dac_chunked(C.c_void_p(rows.ctypes.data), C.c_void_p(out.ctypes.data), C.c_size_t(n), c, ilp)
    assert (buf[:32] == 0xA5).all() and (buf[32 * (n + 1):] == 0xA5).all() and np.array_equal(rows, before)
    return out.reshape(n, 32).copy()


# ------------------------------------------------------------------ the formula on Python integers
def dac_model(X, Y, Z, T):
    """The issue's formula on the values the four coordinates hold; 32 zero bytes where the shared factor is 0 mod p."""
    p = pm.P
    e, f, g, h = 2 * X * Y % p, (Z * Z + pm.D * T * T) % p, (Y * Y + X * X) % p, (Z * Z - pm.D * T * T) % p
    eg, fh = e * g % p, f * h % p
    w = eg * fh % p
    if w == 0:
        return bytes(32)
    wi = pow(w, p - 2, p)
    zinv, tinv = eg * wi % p, fh * wi % p
    magic = pm.INV_SQRT_A_MINUS_D
    if not pm.is_positive(eg * zinv % p):
        e, g, h, magic = g, (p - e) % p, f * pm.SQRT_M1 % p, pm.SQRT_M1
    if not pm.is_positive(h * e * zinv % p):
        g = (p - g) % p
    s = (h - g) * magic * g * tinv % p
    if not pm.is_positive(s):
        s = p - s
    return pm.fe_to_bytes(s)


def model_rows(rows):
    return np.array([list(dac_model(*[H.value(r[5 * k:5 * k + 5]) % pm.P for k in range(4)])) for r in rows], dtype=np.uint8)


def test_formula_against_the_python_model():
    """2 000 seeded curve points from all cosets of the subgroup (a walk P += Q over decoded points, torsion included), each in
    coordinates scaled by a random factor, and the eight-element group E[8] met on the way: the formula gives
    pymodel.ris_compress(2 P) byte for byte, and zeros exactly where that composition gives zeros."""
    rng = random.Random(SEED)
    starts = []
    y = 2
    while len(starts) < 9:
        pt = pm.ed_decompress(int(y).to_bytes(32, "little"))
        if pt is not None:
            starts.append(pt)
        y += 1
    step = pm.ed_scalar_mul(pm.BASEPOINT, rng.randrange(pm.L))
    zeros = 0
    for i in range(2000):
        P = starts[i % len(starts)]
        starts[i % len(starts)] = pm.ed_add(P, step)
        if i % 250 == 0:                                                      # a point of E[8]: L times a decoded point
            P = pm.ed_scalar_mul(P, pm.L)
        lam = rng.randrange(1, pm.P)
        Q = tuple(c * lam % pm.P for c in P)
        want = pm.ris_compress(pm.ed_add(P, P))
        assert dac_model(*Q) == want, i
        zeros += want == bytes(32)
    assert zeros >= 2000 // 250


# ------------------------------------------------------------------ every class, every chunk length
@pytest.fixture(scope="module")
def catalogue(oracle):
    """(rows, class names, expected): every row of every class of tests/point_classes.classes(oracle, 64, seed) interleaved, then
    [0..18] B -- 467 rows, a prime, so every chunk length above 1 leaves a ragged last lane."""
    rows, names = PC.interleave(PC.classes(oracle, 64, SEED))
    mult = [pm.IDENT]
    for _ in range(18):
        mult.append(pm.ed_add(mult[-1], pm.BASEPOINT))
    rows = np.ascontiguousarray(np.concatenate([rows, V.pts_np(mult)]))
    names = names + ["multiple"] * len(mult)
    want = oracle.ris_compress(oracle.ed_double(rows))
    assert len(rows) == 467 and all(len(rows) % c for c in CHUNKS if c > 1)
    return rows, names, want


def test_one_row_per_lane_matches_the_oracle(emul, catalogue):
    rows, names, want = catalogue
    got = dac(emul, rows)
    assert np.array_equal(got, want)
    e8 = [i for i, nm in enumerate(names) if nm == "torsion"] + [len(rows) - 19]          # E[8] and 0 * B
    assert (got[e8] == 0).all() and (got[[i for i in range(len(rows)) if i not in e8 and names[i] in ("subgroup", "multiple")]] != 0).any(axis=1).all()
    assert np.array_equal(model_rows(rows[:64]), want[:64])                               # the Python model on the same bytes


@pytest.mark.parametrize("ilp", [0, 1], ids=["chunked", "lone"])
@pytest.mark.parametrize("c", CHUNKS)
def test_shared_inversions_match_the_oracle_on_every_class(emul, catalogue, c, ilp):
    rows, names, want = catalogue
    assert np.array_equal(dac(emul, rows, c, ilp), want)
    for n in (1, c, c + 1, 2 * c + 1):                                                    # a single lane, full and ragged
        assert np.array_equal(dac(emul, rows[40:40 + n], c, ilp), want[40:40 + n])


@pytest.mark.parametrize("ilp", [0, 1], ids=["chunked", "lone"])
@pytest.mark.parametrize("c", CHUNKS)
def test_hostile_rows_stay_alone_and_get_the_same_bytes_in_every_form(emul, catalogue, c, ilp):
    """tests/hostile_rows point patterns (Z zero by value, all-ones words, random limbs ...) planted at the first, middle and
    last position of lanes: every good row keeps the oracle's bytes, and a hostile row gets what the one-row-per-lane form
    gives it -- which is the formula on the value its words hold.  (The bounds-asserting build takes the patterns whose
    words are below 2^52, as everywhere in this tier.)"""
    rows, names, want = catalogue
    n = 10 * max(c, 8) + 3
    good, gwant = rows[np.arange(n) % len(rows)], want[np.arange(n) % len(rows)]           # c = 64: the catalogue, then again
    hs = H.hostile_set(n, c)
    pats = [(nm, w) for nm, w in H.point_patterns(good[1]) if not emul.checked or H.narrow(w)]
    assert len(pats) >= 10
    clean = dac(emul, good, c, ilp)
    assert np.array_equal(clean, gwant)
    for turn in range(len(pats)):
        a = good.copy()
        planted = H.plant(a, hs, pats, turn)
        assert len(planted) == len(hs)
        got = dac(emul, a, c, ilp)
        H.assert_others_unchanged(clean, got, hs, "ris_double_and_compress c=%d" % c)
        assert np.array_equal(got, dac(emul, a)), "a hostile row's bytes depend on the launch form"
        assert np.array_equal(got[hs], model_rows(a[hs]))
        for i, nm, _ in planted:
            if nm in ("all-zero record", "every coordinate p"):
                assert not got[i].any(), nm


# ------------------------------------------------------------------ the stand-alone sanitizer run
def _record(op, n, c, rows, want):
    return struct.pack("<QQQ", op, n, c) + np.ascontiguousarray(rows, dtype=np.uint64).tobytes() + np.ascontiguousarray(want, dtype=np.uint8).tobytes()


def test_stand_alone_program_under_asan_and_ubsan(tmp_path, catalogue):
    """tests/emul/ris_dac_san.cpp with -fsanitize=address,undefined -fno-sanitize-recover=all and the bounds assertions, on a
    vector file with the catalogue and planted hostile rows for every chunk length; its exit status is the verdict."""
    exe = EB.sanitizer_program("ris_dac_san.cpp", tmp_path, checked=True)
    rows, names, want = catalogue
    blob = _record(1, 96, 0, rows[:96], want[:96])
    for c in CHUNKS:
        n = 10 * max(c, 8) + 3
        a, w = rows[np.arange(n) % len(rows)], want[np.arange(n) % len(rows)]
        hs = H.hostile_set(n, c)
        H.plant(a, hs, [(nm, x) for nm, x in H.point_patterns(a[1]) if H.narrow(x)], c)
        w[hs] = model_rows(a[hs])
        for op in (2, 3):
            blob += _record(op, n, c, a, w)
    blob += struct.pack("<QQQ", 0, 0, 0)
    EB.assert_clean(EB.run_vectors(exe, blob, tmp_path, "vectors.bin"), "rows match")
    # the verdict is a real one: one expected byte changed and the program says so
    bad = bytearray(blob)
    bad[24 + 160 * 96 + 32 * 3 + 5] ^= 1                                                   # byte 5 of row 3 of the first record's encodings
    EB.assert_caught(EB.run_vectors(exe, bad, tmp_path, "wrong.bin"), "row 3 byte 5")
