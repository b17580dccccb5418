"""CPU tier: the device functions behind zc_ed_lincomb_shared and zc_ris_lincomb_shared (zc_shared.hip.h: the partial tables of odd
multiples, the loop over the host's joint schedule, the decode-into-table steps, the fused double-and-encode), built for the host
by tests/emul/shared_lincomb_emul.cpp in the plain and the bounds-asserting (-DZC_CHECK_BOUNDS) build.  The Edwards form is
compared with tests/lincomb_rows.oracle_lincomb as a group element, the wire form byte for byte with
tests/ris_lincomb_rows.oracle_ris_lincomb, both with the scalar vector tiled into every row; the identity the wire form rests on
is also checked on oracle/pymodel.py alone."""
import ctypes as C
import random

import numpy as np
import pytest

from oracle import pymodel as pm
from tests import emul_build as EB
from tests import lincomb_rows as R
from tests import shared_lincomb_rows as SL
from tests import shared_scalar_rows as S

TERMS = [1, 2, 3, 5, 8]
A5 = 0xA5A5A5A5A5A5A5A5


def vectors(t):
    return SL.planted_vectors(t) + SL.edge_vectors(t, S.edge_scalars() + S.random_scalars(2))


@pytest.fixture(scope="module", params=["plain", "checked"])
def emul(request):
    checked = request.param == "checked"
    so = EB.library("shared_lincomb_emul.cpp", checked=checked)
    if so is None:
        pytest.skip("ROCm headers not present")
    lib = C.CDLL(so)
    lib.checked = checked
    return lib


def ed_shared(lib, P, K, ilp=0, in_place=False):
    """The output is framed: nothing outside the n rows may change; neither may the inputs (unless the call is in place)."""
    P = np.ascontiguousarray(P, dtype=np.uint64).copy()
    n, t = P.shape[:2]
    kk = np.array(K, dtype=np.uint64).reshape(t, 5)
    kp = C.c_void_p(kk.ctypes.data)
    if in_place:
        assert t == 1
        lib.emul_ed_lincomb_shared(C.c_void_p(P.ctypes.data), kp, C.c_size_t(t), C.c_void_p(P.ctypes.data), C.c_size_t(n), ilp)
        return P.reshape(n, 20)
    before = P.copy()
    buf = np.full(20 * (n + 2), A5, dtype=np.uint64)
    out = buf[20:20 * (n + 1)]
    lib.emul_ed_lincomb_shared(C.c_void_p(P.ctypes.data), kp, C.c_size_t(t), C.c_void_p(out.ctypes.data), C.c_size_t(n), ilp)
    assert (buf[:20] == A5).all() and (buf[20 * (n + 1):] == A5).all()
    assert np.array_equal(P, before) and np.array_equal(kk, np.array(K, dtype=np.uint64).reshape(t, 5))
    return out.reshape(n, 20).copy()


def ris_shared(lib, E, K, ilp=0, want_ok=True):
    E = np.ascontiguousarray(E, dtype=np.uint8).copy()
    n, t = E.shape[:2]
    kk = np.array(K, dtype=np.uint64).reshape(t, 5)
    okbuf = np.full(n + 2, 0xA5, dtype=np.uint8)
    okp = C.c_void_p(okbuf[1:].ctypes.data) if want_ok else None
    before = E.copy()
    buf = np.full(32 * (n + 2), 0xA5, dtype=np.uint8)
    out = buf[32:32 * (n + 1)].reshape(n, 32)
    lib.emul_ris_lincomb_shared(C.c_void_p(E.ctypes.data), C.c_void_p(kk.ctypes.data), C.c_size_t(t), C.c_void_p(out.ctypes.data), okp, C.c_size_t(n), ilp)
    assert (buf[:32] == 0xA5).all() and (buf[32 * (n + 1):] == 0xA5).all() and np.array_equal(E, before)
    assert okbuf[0] == 0xA5 and okbuf[-1] == 0xA5 and (want_ok or (okbuf == 0xA5).all())
    return out.copy(), okbuf[1:-1].copy()


# ------------------------------------------------------------------ the Edwards form
@pytest.mark.parametrize("t", TERMS)
def test_ed_form_is_the_references_sum_on_every_class(emul, oracle, t):
    """Every class of tests/point_classes in every term (identity, E[8], mixed order, order L, decoded, other coordinates) and the
    planted rows, under the planted vectors and every edge scalar: the oracle's ((k0 P0 + k1 P1) + ...) as a group element."""
    P = SL.point_rows(oracle, t)
    vecs = vectors(t)
    assert sum(len(K) for _, K in vecs) >= 24 + 2 * t
    for vi, (name, K) in enumerate(vecs):
        got = ed_shared(emul, P, K)
        R.assert_same_points(oracle, got, SL.want_ed(oracle, t, K))
        assert (got <= (1 << 52) - 1).all(), name
        if vi % 8 == 0:
            assert np.array_equal(ed_shared(emul, P[:96], K, ilp=1), got[:96]), name             # the form small launches take: the same limbs


@pytest.mark.parametrize("t", [2, 3, 8])
def test_ed_form_planted_rows_are_what_they_are_planted_for(emul, oracle, t):
    P = SL.point_rows(oracle, t)
    ident = np.tile(np.array(S.PC.ident_rows(1)), (len(P), 1))
    by_name = dict(SL.planted_vectors(t))
    got = ed_shared(emul, P, by_name["(k, k, 0..)"])
    assert oracle.ed_eq(got, ident)[list(SL.NEG_ROWS)].all()                                     # k P - k P
    dbl = ed_shared(emul, np.ascontiguousarray(P[list(SL.SAME_ROWS), :1]), [pm.limbs(2 * sum(int(x) << (52 * i) for i, x in enumerate(by_name["(k, k, 0..)"][0])))])
    assert oracle.ed_eq(got[list(SL.SAME_ROWS)], dbl).all()                                      # k P + k P = (2 k) P
    for name, K in SL.planted_vectors(t):
        assert oracle.ed_eq(ed_shared(emul, P[list(SL.IDENT_ROWS)], K), ident[:4]).all(), name   # every point the identity
    assert oracle.ed_eq(ed_shared(emul, P, by_name["all zero"]), ident).all()


def test_one_term_gives_the_limbs_of_the_single_scalar_form(emul, oracle):
    """terms == 1: the same table records and the same schedule as shared_table_build / shared_steps, whatever the entry bound."""
    one = C.CDLL(EB.library("shared_scalar_emul.cpp", checked=emul.checked))
    P, (E, _) = SL.point_rows(oracle, 1), SL.encoding_rows(oracle, 1)
    for k in S.edge_scalars()[::5] + S.random_scalars(1):
        kk = np.array(k, dtype=np.uint64)
        want = np.zeros((len(P), 20), dtype=np.uint64)
        one.emul_ed_scalar_mul_shared(C.c_void_p(P.ctypes.data), C.c_void_p(kk.ctypes.data), C.c_void_p(want.ctypes.data), C.c_size_t(len(P)), 0)
        assert np.array_equal(ed_shared(emul, P, [k]), want)
        assert np.array_equal(ed_shared(emul, P, [k], in_place=True), want)                      # out == points
        wb, wok = np.zeros((len(E), 32), dtype=np.uint8), np.zeros(len(E), dtype=np.uint8)
        one.emul_ris_mul_shared(C.c_void_p(E.ctypes.data), C.c_void_p(kk.ctypes.data), C.c_void_p(wb.ctypes.data), C.c_void_p(wok.ctypes.data), C.c_size_t(len(E)), 0)
        gb, gok = ris_shared(emul, E, [k])
        assert np.array_equal(gb, wb) and np.array_equal(gok, wok)


# ------------------------------------------------------------------ the wire form
@pytest.mark.parametrize("t", TERMS)
def test_wire_form_gives_the_bytes_of_ris_lincomb_with_tiled_scalars(emul, oracle, t):
    """Bytes and ok of every row: elligator images, [0..15] B, the identity's encoding, undecodable rows and junk in every term
    position -- under a zero scalar too (the "zero at j" vectors: the row stays refused)."""
    E, ok_terms = SL.encoding_rows(oracle, t)
    for vi, (name, K) in enumerate(vectors(t)):
        want, wok = SL.want_wire(oracle, t, K)
        got, ok = ris_shared(emul, E, K)
        assert np.array_equal(ok, wok), (name, np.flatnonzero(ok != wok)[:8])
        assert np.array_equal(got, want), (name, np.flatnonzero((got != want).any(axis=1))[:8])
        assert not got[ok == 0].any() and np.array_equal(ok == 1, ok_terms.all(axis=1))
        if name.startswith("zero at "):
            j = int(name.split()[-1])
            assert (ok[ok_terms[:, j] == 0] == 0).all() and (ok_terms[:, j] == 0).any()          # undecodable under a zero scalar
        if vi % 8 == 0:
            for kw in (dict(ilp=1), dict(want_ok=False)):
                assert np.array_equal(ris_shared(emul, E[:120], K, **kw)[0], got[:120]), (name, kw)


@pytest.mark.parametrize("t", [2, 8])
def test_wire_form_identity_sums_leave_as_zero_bytes_with_ok_set(emul, oracle, t):
    E, ok_terms = SL.encoding_rows(oracle, t)
    by_name = dict(SL.planted_vectors(t))
    got, ok = ris_shared(emul, E, by_name["(k, k, 0..)"])
    assert not got[list(SL.NEG_ROWS)].any() and ok[list(SL.NEG_ROWS)].all()
    assert not got[list(SL.IDENT_ROWS)].any() and ok[list(SL.IDENT_ROWS)].all()
    got, ok = ris_shared(emul, E, by_name["all zero"])
    assert not got.any() and np.array_equal(ok == 1, ok_terms.all(axis=1))


def test_the_half_scalar_identity_of_a_sum_on_python_integers():
    """encode(2 sum_j k'_j P_j) = encode(sum_j k_j P_j) with k'_j = (k_j mod L) / 2 mod L for decoded P_j, on oracle/pymodel.py
    alone: every scalar of the list against every other in a two-term sum, and three-term sums drawn from it."""
    rng = random.Random(SL.SEED)
    L = pm.L
    inv2 = (L + 1) // 2
    ks = [0, 1, 2, L - 1, L, L + 1, 2 * L + 5, (1 << 252) - 1, (1 << 256) - 1]
    pts = [pm.ris_decompress(pm.ris_compress(pm.elligator(rng.randrange(pm.P)))) for _ in range(3)]
    assert all(p is not None for p in pts)
    full = [[pm.ed_scalar_mul(p, k) for k in ks] for p in pts]
    half = [[pm.ed_scalar_mul(p, (k % L) * inv2 % L) for k in ks] for p in pts]

    def check(idx):
        a = b = pm.IDENT
        for j, i in enumerate(idx):
            a, b = pm.ed_add(a, full[j][i]), pm.ed_add(b, half[j][i])
        assert pm.ris_compress(pm.ed_add(b, b)) == pm.ris_compress(a), [ks[i] for i in idx]
    for i in range(len(ks)):
        for j in range(len(ks)):
            check((i, j))
    for _ in range(40):
        check(tuple(rng.randrange(len(ks)) for _ in range(3)))
