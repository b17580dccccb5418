"""CPU tier: the device functions behind zc_ris_lincomb_sum (zc_ris_batch.hip.h: ris_sum_pair, ris_sum_row, the sc_sum_*
reduction, ris_sum_store_basepoint), built for the host by tests/emul/ris_sum_emul.cpp in the plain and the bounds-asserting
(-DZC_CHECK_BOUNDS) build and driven as the three kernels drive them.  Expected values: Python integers for every scalar
(tests/ris_sum_rows.py), oracle.zc_ref for the decoded records and the encoded sum, oracle/pymodel.py alone for the smallest
batch.  The sanitizer run is a stand-alone program (tests/emul/ris_sum_san.cpp) replaying a vector file as a child process:
nothing sanitized is loaded here."""
import ctypes as C
import random
import struct

import numpy as np
import pytest

from oracle import pymodel as pm
from tests import emul_build as EB
from tests import ris_lincomb_rows as RR
from tests import ris_sum_rows as RS
from tests import scalar_ext_rows as SX
from tests import vectors as V

SEED = V.SEED + 0x5A70
L = pm.L
BLOCK, PER_LANE, MAX_BLOCKS = 64, 4, 3            # the emulator's reduction geometry: a workgroup's span is 256 rows
VP = C.c_void_p


@pytest.fixture(scope="module", params=["plain", "checked"])
def emul(request):
    checked = request.param == "checked"
    so = EB.library("ris_sum_emul.cpp", checked=checked)
    if so is None:
        pytest.skip("ROCm headers not present")
    lib = C.CDLL(so)
    lib.checked = checked
    return lib


def _ptr(a):
    return VP(a.ctypes.data) if a is not None else None


def pipeline(lib, E, K, KB=None, Z=None, want_ok=True):
    """The three launches on arrays framed with 0xA5 rows: (points, scalars, term flags, ok, t, b).  points and scalars
    hold n t (+ 1) pairs, the base term's last; nothing outside them may change, and no input."""
    E, K = np.ascontiguousarray(E, dtype=np.uint8), np.ascontiguousarray(K, dtype=np.uint64)
    n, t = E.shape[:2]
    pairs, count = n * t, n * t + (KB is not None)
    ins = [a if a is None else np.ascontiguousarray(a, dtype=np.uint64) for a in (KB, Z)]
    before = [a if a is None else a.copy() for a in (E, K) + tuple(ins)]
    fr = lambda rows, width, dt: np.full((rows + 2) * width, 0xA5, dtype=np.uint8).view(dt)
    pts, sc = fr(count, 160, np.uint64), fr(count, 40, np.uint64)
    flags, ok, tt = fr(pairs, 1, np.uint8), fr(n, 1, np.uint8), fr(n, 40, np.uint64)
    P, S = pts[20:20 * (count + 1)], sc[5:5 * (count + 1)]
    F, OK, T = flags[1:pairs + 1], ok[1:n + 1], tt[5:5 * (n + 1)]
    lib.emul_ris_sum_prepare(_ptr(E), _ptr(K), _ptr(ins[1]), _ptr(P), _ptr(S), _ptr(F), C.c_size_t(t), C.c_size_t(pairs))
    base = KB is not None
    lib.emul_ris_sum_rows(_ptr(F), _ptr(S), _ptr(ins[0]), _ptr(ins[1]), _ptr(OK) if want_ok else None, _ptr(T) if base else None,
                          VP(P.ctypes.data + 160 * pairs) if base else None, C.c_size_t(t), C.c_size_t(n))
    b = None
    if base:
        lib.emul_sc_sum(_ptr(T), C.c_size_t(n), VP(S.ctypes.data + 40 * pairs), BLOCK, C.c_size_t(PER_LANE), C.c_size_t(MAX_BLOCKS))
        b = S[5 * pairs:].copy().reshape(1, 5)
    for whole, part in ((pts, P), (sc, S), (flags, F), (ok, OK), (tt, T)):
        w8, lo = whole.view(np.uint8), part.ctypes.data - whole.ctypes.data
        assert (w8[:lo] == 0xA5).all() and (w8[lo + part.nbytes:] == 0xA5).all()
    if not want_ok:
        assert (OK == 0xA5).all()
    if not base:
        assert (T.view(np.uint8) == 0xA5).all()
    for a, was in zip((E, K) + tuple(ins), before):
        assert a is None or np.array_equal(a, was)
    return P.reshape(count, 20).copy(), S.reshape(count, 5).copy(), F.copy(), OK.copy(), (T.reshape(n, 5).copy() if base else None), b


def batch(oracle, n, t, seed, reject=True):
    E = RS.encodings_of_multiples(oracle, n * t, seed).reshape(n, t, 32)
    rows = RS.plant_rejected(oracle, E, seed + 1, every=5) if reject else []
    return E, RS.mixed_scalars(n * t, seed + 2).reshape(n, t, 5), RS.mixed_scalars(n, seed + 3), RS.mixed_scalars(n, seed + 4), rows


@pytest.mark.parametrize("weights", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("base", [False, True], ids=["nobase", "base"])
@pytest.mark.parametrize("n,t", [(1, 1), (3, 2), (40, 1), (33, 7)])
def test_prepare_and_rows_against_python_integers_and_the_oracle(emul, oracle, n, t, base, weights):
    """w_ij, the term flags, the row mask, the zeroed scalars of rejected rows, t_i and b, on raw and canonical patterns."""
    E, K, KB, Z, rejected = batch(oracle, n, t, SEED + 100 * n + t)
    KB, Z = (KB if base else None), (Z if weights else None)
    P, S, F, OK, T, b = pipeline(emul, E, K, KB, Z)
    D, flags = RS.decode_mask(oracle, E)
    ok = flags.all(axis=1)
    assert np.array_equal(F.reshape(n, t) != 0, flags) and np.array_equal(OK, ok.astype(np.uint8)) and set(np.flatnonzero(~ok)) == set(rejected)
    w, tb = RS.weights_and_terms(K, KB, Z)
    want_s = SX.rows([x if ok[i] else 0 for i in range(n) for x in w[i]])
    assert np.array_equal(S[:n * t], want_s)
    want_p = D.reshape(n * t, 20).copy()
    want_p[~flags.reshape(-1)] = V.IDENT_ROW
    assert np.array_equal(P[:n * t], want_p)
    if base:
        assert np.array_equal(T, SX.rows([x if ok[i] else 0 for i, x in enumerate(tb)]))
        assert np.array_equal(b, SX.rows([sum(x for i, x in enumerate(tb) if ok[i]) % L]))
        assert np.array_equal(P[n * t], RR.basepoint_rows(1)[0])
    # the MSM of what the passes wrote is the expected sum
    got = bytes(oracle.ris_compress(oracle.msm_naive_mt(P, S))[0])
    assert got == RS.expected(oracle, E, K, KB, Z)[0]
    if (n, t) == (3, 2):
        assert (got, OK.tolist()) == (lambda r: (r[0], r[1].tolist()))(RS.expected_pymodel(E, K, KB, Z))


def test_ok_may_be_null_and_all_rejected_rows_leave_only_zero_scalars(emul, oracle):
    E, K, KB, Z, _ = batch(oracle, 6, 2, SEED + 7, reject=False)
    for i in range(6):
        E[i, i % 2] = RS.bad_encodings(oracle, E[i, i % 2], SEED + 8 + i)[i % 4]
    P, S, F, OK, T, b = pipeline(emul, E, K, KB, Z, want_ok=False)
    assert not S.any() and not T.any() and not b.any()
    assert bytes(oracle.ris_compress(oracle.msm_naive_mt(P, S))[0]) == RS.ZERO32 == RS.expected(oracle, E, K, KB, Z)[0]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 1000])
def test_reduction_is_the_python_sum_in_every_geometry(emul, n):
    """n up to one past a wave, one past a workgroup's span (257 > 64 x 4: two partials meet in the second launch) and beyond the
    workgroup cap (1000 > 3 x 256: the lanes stride); also the product's own geometry, and a lone workgroup."""
    rng = random.Random(SEED + n)
    vals = [rng.randrange(L) for _ in range(n)]
    for idx, v in enumerate([0, L - 1, L - 1, 1, 0]):
        if idx < n:
            vals[(7 * idx) % n] = v
    t = SX.rows(vals)
    want = SX.rows([sum(vals) % L])
    for block, per_lane, max_blocks in ((BLOCK, PER_LANE, MAX_BLOCKS), (256, 4, 1024), (2, 1, 1000), (64, 1, 1)):
        out = np.full(15, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        emul.emul_sc_sum(_ptr(t), C.c_size_t(n), VP(out.ctypes.data + 40), block, C.c_size_t(per_lane), C.c_size_t(max_blocks))
        assert np.array_equal(out[5:10].reshape(1, 5), want), (block, per_lane, max_blocks)
        assert (out[:5] == 0xA5A5A5A5A5A5A5A5).all() and (out[10:] == 0xA5A5A5A5A5A5A5A5).all()


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
def test_base_term_of_raw_patterns_is_the_python_sum(emul, oracle, n):
    """b through the rows pass and the reduction from raw weights and base scalars (tests/scalar_ext_rows.py patterns: values at or
    above L, words with bits at or above 2^52, multiples of L), every fifth row rejected."""
    pats = np.array([w for _, w in SX.zero_patterns()] + list(SX.invert_edges()) + [[SX.ALL_ONES] * 5], dtype=np.uint64)
    KB, Z = RS.mixed_scalars(n, SEED + 300 + n), RS.mixed_scalars(n, SEED + 400 + n)
    for i in range(n):
        if i % 2:
            KB[i] = pats[i % len(pats)]
        if i % 3 == 0:
            Z[i] = pats[(i // 3) % len(pats)]
    E = np.zeros((n, 1, 32), dtype=np.uint8)                                           # the identity's encoding
    bad = RR.le32(pm.P + 5)
    E[4::5, 0] = bad
    K = np.zeros((n, 1, 5), dtype=np.uint64)
    _, S, _, OK, T, b = pipeline(emul, E, K, KB, Z)
    ok = [i % 5 != 4 for i in range(n)]
    assert OK.tolist() == [int(o) for o in ok]
    terms = [zv * kv % L if o else 0 for zv, kv, o in zip(SX.values(Z), SX.values(KB), ok)]
    assert np.array_equal(T, SX.rows(terms)) and np.array_equal(b, SX.rows([sum(terms) % L]))


# ------------------------------------------------------------------ the stand-alone sanitizer run
def _record(E, K, KB, Z, want_p, want_s, want_ok):
    n, t = E.shape[:2]
    blob = struct.pack("<QQQQ", 1, n, t, (1 if KB is not None else 0) | (2 if Z is not None else 0))
    for a, dt in ((E, np.uint8), (K, np.uint64), (KB, np.uint64), (Z, np.uint64), (want_p, np.uint64), (want_s, np.uint64), (want_ok, np.uint8)):
        if a is not None:
            blob += np.ascontiguousarray(a, dtype=dt).tobytes()
    return blob


def test_stand_alone_program_under_asan_and_ubsan(tmp_path, oracle):
    """tests/emul/ris_sum_san.cpp with -fsanitize=address,undefined -fno-sanitize-recover=all and the bounds assertions, on a
    vector file of batches with and without base term and weights; its exit status is the verdict."""
    exe = EB.sanitizer_program("ris_sum_san.cpp", tmp_path, checked=True)
    blob, first = b"", None
    for n, t, base, weights in ((1, 1, False, False), (3, 2, True, True), (65, 1, True, False), (300, 2, True, True), (20, 7, False, True)):
        E, K, KB, Z, _ = batch(oracle, n, t, SEED + 900 + n)
        # (the bounds-asserting build takes words below 2^52, as everywhere in this tier)
        K, KB, Z = K & np.uint64(SX.M52), (KB & np.uint64(SX.M52) if base else None), (Z & np.uint64(SX.M52) if weights else None)
        P, s, ok = RS.msm_pairs(oracle, E, K, KB, Z)
        D, flags = RS.decode_mask(oracle, E)
        w, tb = RS.weights_and_terms(K, KB, Z)
        want_p = D.reshape(n * t, 20).copy()
        want_p[~flags.reshape(-1)] = V.IDENT_ROW
        want_s = [x if ok[i] else 0 for i in range(n) for x in w[i]]
        if base:
            want_p = np.concatenate([want_p, RR.basepoint_rows(1)])
            want_s.append(s[-1])
        first = first or len(blob) + 32 + E.nbytes + K.nbytes + (KB.nbytes if base else 0) + (Z.nbytes if weights else 0)
        blob += _record(E, K, KB, Z, want_p, SX.rows(want_s), ok)
    blob += struct.pack("<QQQQ", 0, 0, 0, 0)
    EB.assert_clean(EB.run_vectors(exe, blob, tmp_path, "vectors.bin"), "rows match")
    # the verdict is a real one: one expected byte changed and the program says so
    bad = bytearray(blob)
    bad[first + 8] ^= 1                                                                  # in X of the first record's first expected point
    EB.assert_caught(EB.run_vectors(exe, bad, tmp_path, "wrong.bin"), "points")
