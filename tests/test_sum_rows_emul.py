"""CPU tier: the device functions behind the point sums (zc_sum.hip.h: sum_slice_fold, sum_wire_slice_fold, sum_tree_pair and the
partial records, on the plan of zc_sum_plan.h), built for the host by tests/emul/sum_rows_emul.cpp in the plain and the
bounds-asserting (-DZC_CHECK_BOUNDS) build.  The Edwards form must be limb-identical to tests/sum_rows.py: model_sum (the oracle's
ed_add in the documented order), the wire form byte-identical to the oracle's decompress / add / ris_compress with the expected
accept bits, for every term count of the GPU tier.  The sanitizer run is a stand-alone program (tests/emul/sum_rows_san.cpp)
replaying a vector file as a child process: nothing sanitized is loaded here."""
import ctypes as C
import struct

import numpy as np
import pytest

from tests import emul_build as EB
from tests import sum_rows as SR

SHORT_N, LONG_N = 257, 3


@pytest.fixture(scope="module", params=["plain", "checked"])
def emul(request):
    so = EB.library("sum_rows_emul.cpp", checked=request.param == "checked")
    if so is None:
        pytest.skip("ROCm headers not present")
    return SR.Emul(C.CDLL(so))


def _n(terms):
    return LONG_N if terms in SR.LONG_TERMS else SHORT_N


def test_the_rows_are_what_the_issue_asks_for(oracle):
    assert [SR.parts(t) for t in (0, 1, 32, 33, 47, 48, 4095, 4096, 8191, 8192, 8197)] == [1, 1, 1, 2, 2, 2, 128, 256, 256, 512, 512]
    assert 8197 % 512 != 0 and 47 % 2 != 0                                              # uneven slices, in one kernel and in two
    P = SR.points(oracle, 64, 8)
    assert oracle.ed_is_valid(np.ascontiguousarray(P.reshape(-1, 20))).all() and (P <= SR.M52).all()
    assert np.array_equal(P[1, 0], P[1, 7]) and SR.PC.is_identity(oracle, P[7]).all() and SR.PC.is_identity(oracle, P[5, ::3]).all()
    assert SR.PC.is_identity(oracle, oracle.ed_add(np.ascontiguousarray(P[2, 0:1]), np.ascontiguousarray(P[2, 1:2])))[0]
    assert np.array_equal(SR.points(oracle, 3, 8), P[:3])                               # prefixes of one another
    enc, ok = SR.encodings(oracle, 64, 8)
    assert ok.tolist() == [0 if i % 8 in (1, 3, 6) else 1 for i in range(64)]
    for i, j in ((1, 0), (3, 4), (6, 7)):
        assert oracle.ris_decompress(np.ascontiguousarray(enc[i]))[1].tolist() == [0 if t == j else 1 for t in range(8)]
    assert not SR.want_wire(oracle, 64, 8)[0][7].any() and SR.want_wire(oracle, 64, 8)[1][7] == 1      # an identity sum: zero bytes, accepted


@pytest.mark.parametrize("terms", SR.SHORT_TERMS + SR.LONG_TERMS)
def test_ed_form_has_the_models_limbs(emul, oracle, terms):
    n = _n(terms)
    pts = SR.points(oracle, n, terms)
    got = emul.ed(pts)
    want = SR.want_ed(oracle, n, terms)
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:8]
    for i in (0, 1, 2, n - 1):                                                          # the limbs of a row do not change with the rows beside it
        assert np.array_equal(emul.ed(pts[i:i + 1]), got[i:i + 1])
    if terms == 1:
        assert np.array_equal(got, pts[:, 0])                                           # the point itself, not identity + point
    if terms == 0:
        assert np.array_equal(got, SR.PC.ident_rows(n))


@pytest.mark.parametrize("terms", SR.SHORT_TERMS + SR.LONG_TERMS)
def test_wire_form_gives_the_oracles_bytes_and_accept_bits(emul, oracle, terms):
    n = _n(terms)
    enc, _ = SR.encodings(oracle, n, terms)
    want, wok = SR.want_wire(oracle, n, terms)
    got, ok = emul.wire(enc)
    assert np.array_equal(ok, wok) and np.array_equal(got, want), (np.flatnonzero(ok != wok)[:8], np.flatnonzero((got != want).any(axis=1))[:8])
    assert np.array_equal(emul.wire(enc, with_ok=False)[0], want)                       # ok = NULL
    for i in (0, 1, n - 1):
        one, ok1 = emul.wire(enc[i:i + 1])
        assert np.array_equal(one, got[i:i + 1]) and ok1[0] == wok[i]


def test_wire_form_is_the_compression_of_the_edwards_form(emul, oracle):
    for terms in (3, 33, 4096):
        n = _n(terms)
        enc, ok = SR.encodings(oracle, n, terms)
        pts, _ = oracle.mt(oracle.ris_decompress, np.ascontiguousarray(enc.reshape(-1, 32)))
        ed = emul.ed(pts.reshape(n, terms, 20))
        want = oracle.mt(oracle.ris_compress, ed)
        want[ok == 0] = 0
        assert np.array_equal(emul.wire(enc)[0], want)


def test_the_folds_decoder_is_ris_decompress(emul, oracle):
    """sum_ris_decode is ris_decompress with sqrt_ratio_i written out for u = 1: on every encoding of the rows, on the
    undecodable ones, on hostile bytes and on seeded random bytes the verdict and every canonical limb of the point agree."""
    rng = np.random.default_rng(SR.SEED)
    rnd = rng.integers(0, 256, size=(4096, 32), dtype=np.uint8)
    rnd[::2, 31] &= 0x7F
    edge = np.array([list(int(v % (1 << 256)).to_bytes(32, "little")) for v in (0, 1, 2, SR.HR.pm.P - 1, SR.HR.pm.P, SR.HR.pm.P + 1, (SR.HR.pm.P - 1) // 2,
                                                                                (SR.HR.pm.P + 1) // 2, (1 << 255) - 1, 1 << 255, (1 << 256) - 1)], dtype=np.uint8)
    sets = [SR.encodings(oracle, 257, 47)[0], np.stack(SR.undecodable(oracle)), SR.FBROWS(oracle), rnd, edge]
    for rows in sets:
        assert emul.decode_differs(rows) == 0
    assert 0 < oracle.ris_decompress(rnd)[1].sum() < len(rnd)                          # both verdicts occur among the random bytes


def test_stand_alone_program_under_asan_and_ubsan(tmp_path, oracle):
    """tests/emul/sum_rows_san.cpp with -fsanitize=address,undefined -fno-sanitize-recover=all: inputs and outputs in heap blocks of
    exactly their size, one record per term count on either side of every plan boundary; its exit status is the verdict."""
    exe = EB.sanitizer_program("sum_rows_san.cpp", tmp_path)
    blob, rows, records = b"", 0, 0
    for terms in (0, 1, 3, 32, 33, 47, 4096, 8197):
        n = 2 if terms in SR.LONG_TERMS else 9
        enc, ok = SR.encodings(oracle, n, terms)
        blob += struct.pack("<3Q", 1, terms, n) + SR.points(oracle, n, terms).tobytes() + np.ascontiguousarray(SR.want_ed(oracle, n, terms)).tobytes()
        blob += enc.tobytes() + np.ascontiguousarray(SR.want_wire(oracle, n, terms)[0]).tobytes() + np.ascontiguousarray(ok).astype("<u8").tobytes()
        rows += n
        records += 1
    blob += struct.pack("<Q", 0)
    EB.assert_clean(EB.run_vectors(exe, blob, tmp_path, "vectors.bin"), "%d records, %d rows match" % (records, rows))
    bad = bytearray(blob)
    bad[-8 - 8 * 2 - 1] ^= 1                                                            # the last byte of the last expected encoding
    EB.assert_caught(EB.run_vectors(exe, bad, tmp_path, "wrong.bin"), "record %d: row 1: the encoding differs" % (records - 1))
