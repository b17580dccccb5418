"""CPU tier: the device functions behind zc_ed_scalar_mul_shared and zc_ris_mul_shared (zc_shared.hip.h: the table of odd
multiples, the loop over the host's schedule, the fused double-and-encode), built for the host by tests/emul/
shared_scalar_emul.cpp in the plain and the bounds-asserting (-DZC_CHECK_BOUNDS) build, with the lane's table in a local array
(table_ptr).  Every row is compared with the C oracle (ed_scalar_mul, ris_roundtrip_mul); the k / 2 identity the wire form
rests on is also checked on Python integers against oracle/pymodel.py, so both oracles are on record."""
import ctypes as C
import random

import numpy as np
import pytest

from oracle import pymodel as pm
from tests import emul_build as EB
from tests import hostile_rows as H
from tests import shared_scalar_rows as S

SCALARS = S.edge_scalars() + S.random_scalars(8)


@pytest.fixture(scope="module", params=["plain", "checked"])
def emul(request):
    checked = request.param == "checked"
    so = EB.library("shared_scalar_emul.cpp", checked=checked)
    if so is None:
        pytest.skip("ROCm headers not present")
    lib = C.CDLL(so)
    lib.checked = checked
    return lib


def ed_shared(lib, rows, k, ilp=0, in_place=False):
    """The output is framed: nothing outside the n rows may change; neither may the inputs (unless the call is in place)."""
    rows = np.ascontiguousarray(rows, dtype=np.uint64).copy()
    n = len(rows)
    kk = np.array(k, dtype=np.uint64)
    if in_place:
        lib.emul_ed_scalar_mul_shared(C.c_void_p(rows.ctypes.data), C.c_void_p(kk.ctypes.data), C.c_void_p(rows.ctypes.data), C.c_size_t(n), ilp)
        return rows
    before = rows.copy()
    buf = np.full(20 * (n + 2), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    out = buf[20:20 * (n + 1)]
    lib.emul_ed_scalar_mul_shared(C.c_void_p(rows.ctypes.data), C.c_void_p(kk.ctypes.data), C.c_void_p(out.ctypes.data), C.c_size_t(n), ilp)
    assert (buf[:20] == 0xA5A5A5A5A5A5A5A5).all() and (buf[20 * (n + 1):] == 0xA5A5A5A5A5A5A5A5).all()
    assert np.array_equal(rows, before) and [int(x) for x in kk] == [int(x) for x in k]
    return out.reshape(n, 20).copy()


def ris_shared(lib, enc, k, ilp=0, in_place=False, want_ok=True):
    enc = np.ascontiguousarray(enc, dtype=np.uint8).copy()
    n = len(enc)
    kk = np.array(k, dtype=np.uint64)
    okbuf = np.full(n + 2, 0xA5, dtype=np.uint8)
    okp = C.c_void_p(okbuf[1:].ctypes.data) if want_ok else None
    if in_place:
        lib.emul_ris_mul_shared(C.c_void_p(enc.ctypes.data), C.c_void_p(kk.ctypes.data), C.c_void_p(enc.ctypes.data), okp, C.c_size_t(n), ilp)
        out = enc
    else:
        before = enc.copy()
        buf = np.full(32 * (n + 2), 0xA5, dtype=np.uint8)
        out = buf[32:32 * (n + 1)].reshape(n, 32)
        lib.emul_ris_mul_shared(C.c_void_p(enc.ctypes.data), C.c_void_p(kk.ctypes.data), C.c_void_p(out.ctypes.data), okp, C.c_size_t(n), ilp)
        assert (buf[:32] == 0xA5).all() and (buf[32 * (n + 1):] == 0xA5).all() and np.array_equal(enc, before)
        out = out.copy()
    assert okbuf[0] == 0xA5 and okbuf[-1] == 0xA5 and (want_ok or (okbuf == 0xA5).all())
    return out, okbuf[1:-1].copy()


# ------------------------------------------------------------------ the Edwards form
@pytest.mark.parametrize("ki", range(len(SCALARS)))
def test_ed_form_is_the_references_group_element_on_every_class(emul, oracle, ki):
    """identity, E[8], mixed order, order L, decoded points, other coordinates, 200 seeded points: equal under ==, identical
    encodings; torsion and mixed-order points are multiplied by the integer (the oracle's double_and_add does just that)."""
    k = SCALARS[ki]
    rows, names = S.point_pool(oracle)
    want = S.want_ed(oracle, rows, k)
    got = ed_shared(emul, rows, k)
    assert oracle.ed_eq(got, want).all(), np.flatnonzero(oracle.ed_eq(got, want) == 0)[:8]
    (gb, gok), (wb, wok) = oracle.ed_compress(got), oracle.ed_compress(want)
    assert np.array_equal(gb, wb) and np.array_equal(gok, wok)
    assert (got <= (1 << 52) - 1).all() and oracle.mt(oracle.ed_is_valid, got).all()
    if ki % 6 == 0:
        assert np.array_equal(ed_shared(emul, rows[:96], k, ilp=1), got[:96])            # the form small launches take: the same limbs
        assert np.array_equal(ed_shared(emul, rows[:96], k, in_place=True), got[:96])    # out == p


def test_ed_form_multiplies_mixed_order_points_by_the_integer_not_by_k_mod_l(emul, oracle):
    rows, names = S.point_pool(oracle)
    mixed = np.array([i for i, nm in enumerate(names) if nm.startswith("order_")])
    a = ed_shared(emul, rows[mixed], pm.limbs(pm.L + 1))
    b = ed_shared(emul, rows[mixed], pm.limbs(1))
    assert not oracle.ed_eq(a, b).any() and oracle.ed_eq(b, rows[mixed]).all()


def test_ed_form_hostile_rows_get_deterministic_garbage_for_their_own_row(emul, oracle):
    """tests/hostile_rows point patterns among good rows: every good row keeps its result, a hostile row's limbs are the same in
    both multiplier forms and on a second run.  (The bounds-asserting build takes the patterns whose words are below 2^52.)"""
    rows, _ = S.point_pool(oracle)
    k = SCALARS[-1]
    good = rows[:64].copy()
    clean = ed_shared(emul, good, k)
    pats = [(nm, w) for nm, w in H.point_patterns(good[1]) if not emul.checked or H.narrow(w)]
    assert len(pats) >= 10
    a = good.copy()
    where = [3 * j + 1 for j in range(len(pats))]
    for i, (_, w) in zip(where, pats):
        a[i] = np.array(w, dtype=np.uint64)
    got = ed_shared(emul, a, k)
    H.assert_others_unchanged(clean, got, where, "ed_scalar_mul_shared")
    assert np.array_equal(got, ed_shared(emul, a, k)) and np.array_equal(got, ed_shared(emul, a, k, ilp=1))


# ------------------------------------------------------------------ the wire form
@pytest.mark.parametrize("ki", range(len(SCALARS)))
def test_wire_form_gives_the_bytes_of_roundtrip_mul(emul, oracle, ki):
    """Bytes and ok for every row: elligator images, [0..15] B, encodings of the identity, undecodable rows, junk."""
    k = SCALARS[ki]
    enc = S.encoding_pool(oracle)
    want, wok = S.want_wire(oracle, enc, k)
    got, ok = ris_shared(emul, enc, k)
    assert np.array_equal(ok, wok), np.flatnonzero(ok != wok)[:8]
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:8]
    assert not got[ok == 0].any()
    if ki % 6 == 0:
        for kw in (dict(ilp=1), dict(in_place=True), dict(want_ok=False)):
            assert np.array_equal(ris_shared(emul, enc[:120], k, **kw)[0], got[:120]), kw


def test_wire_form_identity_products_leave_as_zero_bytes_with_ok_set(emul, oracle):
    enc = S.encoding_pool(oracle)
    dec = oracle.ris_decompress(enc)[1] == 1
    for k in (pm.limbs(0), pm.limbs(pm.L), pm.limbs(2 * pm.L)):
        got, ok = ris_shared(emul, enc, k)
        assert not got.any() and np.array_equal(ok == 1, dec)
    got, ok = ris_shared(emul, enc, pm.limbs(1))
    assert np.array_equal(got[dec], enc[dec])                                             # k = 1: k' = (L + 1) / 2, and the bytes come back


def test_the_half_scalar_identity_on_python_integers():
    """compress(k P) = compress(2 ((k mod L) 2^-1 mod L) P) for decoded P, on oracle/pymodel.py alone: elligator images and small
    multiples of the basepoint, re-encoded and decoded; scalars on both sides of L and the longest patterns."""
    rng = random.Random(S.SEED)
    encs = [pm.ris_compress(pm.elligator(rng.randrange(pm.P))) for _ in range(20)]
    acc = pm.IDENT
    for _ in range(6):
        encs.append(pm.ris_compress(acc))
        acc = pm.ed_add(acc, pm.BASEPOINT)
    L = pm.L
    inv2 = (L + 1) // 2
    for e in encs:
        P = pm.ris_decompress(e)
        assert P is not None
        for k in (0, 1, 2, L - 1, L, L + 1, 2 * L + 5, (1 << 252) - 1, (1 << 256) - 1, rng.randrange(1 << 252)):
            half = pm.ed_scalar_mul(P, (k % L) * inv2 % L)
            assert pm.ris_compress(pm.ed_add(half, half)) == pm.ris_compress(pm.ed_scalar_mul(P, k)), (e.hex(), k)
