"""CPU tier: the device functions behind zc_sc_from_bytes_wide / zc_sc_from_bytes_mod_order, zc_sc_muladd and zc_sc_invert
(zc_arith.hip.h: sc_reduce_words, sc_muladd_limbs52; zc_curve.hip.h: sc_invert_limbs52, mod_invert_chunk<ModL>), built for the
host by tests/emul/scalar_ext_emul.cpp in the plain and the bounds-asserting (-DZC_CHECK_BOUNDS) build.  None of it is in the
reference, so every row is compared with Python integers (tests/scalar_ext_rows.py).  The sanitizer run is a stand-alone
program (tests/emul/scalar_ext_san.cpp) replaying a vector file as a child process: nothing sanitized is loaded here."""
import ctypes as C
import struct

import numpy as np
import pytest

from tests import emul_build as EB
from tests import hostile_rows as H
from tests import scalar_ext_rows as S
from tests import vectors as V

CHUNKS = [1, 2, 3, 16, 64]


@pytest.fixture(scope="module", params=["plain", "checked"])
def emul(request):
    so = EB.library("scalar_ext_emul.cpp", checked=request.param == "checked")
    if so is None:
        pytest.skip("ROCm headers not present")
    return C.CDLL(so)


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def reduce_bytes(lib, b, offset=0):
    """offset: the records start that many bytes into a buffer (an unaligned caller pointer)."""
    n, width = b.shape
    buf = np.zeros(n * width + 8, dtype=np.uint8)
    buf[offset:offset + n * width] = b.reshape(-1)
    out = np.zeros((n, 5), dtype=np.uint64)
    fn = lib.emul_sc_from_bytes_wide if width == 64 else lib.emul_sc_from_bytes_mod_order
    fn(C.c_void_p(buf.ctypes.data + offset), p(out), C.c_size_t(n))
    return out


def muladd(lib, a, b, c):
    out = np.zeros_like(a)
    lib.emul_sc_muladd(p(a), p(b), p(c), p(out), C.c_size_t(len(a)))
    return out


def invert(lib, a, c=0, ilp=0):
    """c = 0: one inversion per row (k_sc_invert); else the shared inversions at c rows per lane."""
    a = np.ascontiguousarray(a)
    out, ok = np.full_like(a, 0xA5A5A5A5), np.full(len(a), 7, dtype=np.uint8)
    if c == 0:
        lib.emul_sc_invert(p(a), p(out), p(ok), C.c_size_t(len(a)))
    else:
        lib.emul_sc_invert_chunked(p(a), p(out), p(ok), C.c_size_t(len(a)), c, ilp)
    return out, ok


def sc_mul(lib, a, b):
    out = np.zeros_like(a)
    lib.emul_sc_mul(p(a), p(b), p(out), C.c_size_t(len(a)))
    return out


ONE = np.array([1, 0, 0, 0, 0], dtype=np.uint64)


@pytest.mark.parametrize("width", [64, 32])
def test_reduction_of_arbitrary_bytes(emul, width):
    """0, 1, L - 1, L, L + 1, 2^256 - 1, 2^256, 2^256 + L, 2^511, 2^512 - 1, k L for k = 2, 255, 2^256, 2^262 (those that fit the
    width), every single-bit input and 4096 random rows: out = v mod L, canonical, from an aligned and an odd address."""
    vals = S.reduction_values(width, 4096, V.SEED + 0x5C01 + width)
    assert len(vals) == 4096 + 8 * width + len([v for v in S.wide_edges() if v < 1 << 8 * width]) and (width == 32 or 2**262 * S.L in vals)
    want = S.canon_rows(vals)
    b = S.to_bytes(vals, width)
    assert np.array_equal(reduce_bytes(emul, b), want)
    assert np.array_equal(reduce_bytes(emul, b, offset=1), want)
    if width == 32:                                                               # the 32-byte form is the wide one with hi = 0
        wide = np.concatenate([b, np.zeros_like(b)], axis=1)
        assert np.array_equal(reduce_bytes(emul, wide), want)


def test_muladd_operand_families(emul):
    a, b, c = S.muladd_families(2048, V.SEED + 0x5C02)
    want = S.muladd_expected(a, b, c)
    got = muladd(emul, a, b, c)
    assert np.array_equal(got, want)
    assert (want[-1] == 0).all() and (want[-4] == 0).all()                        # a b + (L - 1) = L
    # the composition the library offered before, on the emulated multiplier: a b, then + c in integers
    canon = [i for i in range(len(a)) if max(S.values(a[i:i + 1]) + S.values(b[i:i + 1]) + S.values(c[i:i + 1])) < S.L
             and (a[i] | b[i] | c[i]).max() <= S.M52]
    assert len(canon) >= 2048
    prod = sc_mul(emul, a[canon], b[canon])
    assert np.array_equal(S.canon_rows([x + y for x, y in zip(S.values(prod), S.values(c[canon]))]), want[canon])


def test_single_inversion(emul):
    """1, 2, L - 1, L - 2, (L + 1) / 2, the non-canonical L + 1 (-> 1) and 2^260 - 1, 2048 random rows, every zero-by-value
    pattern; a a^-1 = 1 also on the emulated multiplier."""
    zeros = np.array([w for _, w in S.zero_patterns()], dtype=np.uint64)
    a = np.concatenate([S.invert_edges(), S.random_invert_rows(2048, V.SEED + 0x5C03), zeros])
    want, wok = S.invert_expected(a)
    got, ok = invert(emul, a)
    assert np.array_equal(got, want) and np.array_equal(ok, wok)
    assert list(got[5]) == [1, 0, 0, 0, 0] and ok[-len(zeros):].tolist() == [0] * len(zeros) and ok[:-len(zeros)].all()
    nz = ok == 1
    assert (sc_mul(emul, a[nz], got[nz]) == ONE).all()


@pytest.mark.parametrize("ilp", [0, 1], ids=["chunked", "lone"])
@pytest.mark.parametrize("c", CHUNKS)
def test_shared_inversions_over_a_ragged_count(emul, c, ilp):
    n = 5 * max(c, 8) + 3                                                         # the last chunk is ragged
    a = S.random_invert_rows(n, V.SEED + 0x5C10 + c)
    a[:7] = S.invert_edges()
    want, wok = S.invert_expected(a)
    got, ok = invert(emul, a, c, ilp)
    assert np.array_equal(got, want) and np.array_equal(ok, wok) and ok.all()
    assert (sc_mul(emul, a, got) == ONE).all()


@pytest.mark.parametrize("ilp", [0, 1], ids=["chunked", "lone"])
@pytest.mark.parametrize("c", CHUNKS)
def test_rows_that_are_zero_by_value_stay_out_of_the_shared_product(emul, c, ilp):
    """0, L, 2L, 255L, 2047L and a word of high bits only at the first, middle and last position of a chunk (the set
    tests/hostile_rows.py constructs and checks from the launch geometry): those rows give out = 0, ok = 0, every other row is
    exact -- and identical to the same batch with the hostile rows replaced by 1."""
    n = 10 * max(c, 8) + 3
    pats = S.zero_patterns()
    hs = H.hostile_set(n, c)
    for turn in range(len(pats)):
        a = S.random_invert_rows(n, V.SEED + 0x5C20 + c)
        clean = a.copy()
        clean[hs] = ONE
        planted = H.plant(a, hs, pats, turn)
        assert len(planted) == len(hs)
        want, wok = S.invert_expected(a)
        got, ok = invert(emul, a, c, ilp)
        assert np.array_equal(got, want) and np.array_equal(ok, wok)
        assert (got[hs] == 0).all() and (ok[hs] == 0).all() and ok.sum() == n - len(hs)
        H.assert_others_unchanged(invert(emul, clean, c, ilp), (got, ok), hs, "sc_invert c=%d" % c)
        keep = H.clean_mask(n, hs)
        assert (sc_mul(emul, a[keep], got[keep]) == ONE).all()


# ------------------------------------------------------------------ the stand-alone sanitizer run
def _record(op, n, c, *arrays):
    out = struct.pack("<QQQ", op, n, c)
    for arr in arrays:
        raw = np.ascontiguousarray(arr).tobytes()
        out += raw + b"\0" * (-len(raw) % 8)
    return out


def test_stand_alone_program_under_asan_and_ubsan(tmp_path):
    """tests/emul/scalar_ext_san.cpp with -fsanitize=address,undefined -fno-sanitize-recover=all and the bounds assertions, on a
    vector file with inputs and expected outputs of every family above; its exit status is the verdict."""
    exe = EB.sanitizer_program("scalar_ext_san.cpp", tmp_path, checked=True)
    blob = b""
    for width, op in ((64, 1), (32, 2)):
        vals = S.reduction_values(width, 512, V.SEED + 0x5C31 + width)
        blob += _record(op, len(vals), 0, S.to_bytes(vals, width), S.canon_rows(vals))
    a, b, c = S.muladd_families(512, V.SEED + 0x5C32)
    blob += _record(3, len(a), 0, a, b, c, S.muladd_expected(a, b, c))
    zeros = np.array([w for _, w in S.zero_patterns()], dtype=np.uint64)
    a = np.concatenate([S.invert_edges(), S.random_invert_rows(256, V.SEED + 0x5C33), zeros])
    blob += _record(4, len(a), 0, a, *S.invert_expected(a))
    pats = S.zero_patterns()
    for ci in CHUNKS:
        n = 10 * max(ci, 8) + 3
        a = S.random_invert_rows(n, V.SEED + 0x5C34 + ci)
        H.plant(a, H.hostile_set(n, ci), pats, ci)
        for op in (5, 6):
            blob += _record(op, n, ci, a, *S.invert_expected(a))
    blob += struct.pack("<QQQ", 0, 0, 0)
    EB.assert_clean(EB.run_vectors(exe, blob, tmp_path, "vectors.bin"), "rows match")
    # the verdict is a real one: one expected limb changed and the program says so
    bad = bytearray(blob)
    bad[24 + 64 * (len(S.reduction_values(64, 512, 0))) + 5 * 8 * 3] ^= 1         # limb 0 of row 3 of the first record's expected values
    EB.assert_caught(EB.run_vectors(exe, bad, tmp_path, "wrong.bin"), "row 3 limb 0")
