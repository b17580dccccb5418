"""GPU tier: zc_ed_lincomb_shared and zc_ris_lincomb_shared through the C ABI against the oracle (zc_ref) and against the calls
they replace with the scalar vector tiled into every row.  Host arrays and device tensors, batch sizes on both sides of a wave
and of a workgroup, term counts 1, 2, 3, 5 and 8 (one unit, two, an odd count, the first past four, the ring's eight-unit
slot), undecodable terms in every position, planted rows (P1 = -P0, P1 = P0, identities), framed buffers, the caller's k
overwritten right after the call, shrunken table rings, one hostile row among good ones, and the argument checks.  The rows come
from the pools of tests/shared_scalar_rows.py (at most 331 distinct rows) as tests/shared_lincomb_rows.py combines them, repeated
for longer batches; the oracle's answers are cached per pool and scalar."""
import ctypes as C

import numpy as np
import pytest

from oracle import pymodel as pm
from tests import framed_buffers as FB
from tests import hostile_rows as H
from tests import shared_lincomb_rows as SL
from tests import shared_scalar_rows as S
from tests import vectors as V

pytestmark = pytest.mark.gpu

ED, RIS = "zc_ed_lincomb_shared", "zc_ris_lincomb_shared"
SIZES = [1, 63, 65, 257, 1000]
TERMS = [1, 2, 3, 5, 8]
ZC_ERR_BAD_ARG, ZC_ERR_MIXED_MEM = -1, -5


@pytest.fixture(scope="module")
def eng():
    import dusk_zerocaf_amd as z
    e = z.Engine()
    yield e
    e.close()


def dev(x):
    import torch
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x if x.dtype == np.uint8 else x.view(np.int64)).cuda()


def host(t):
    if isinstance(t, np.ndarray):
        return t
    a = t.cpu().numpy()
    return a if a.dtype == np.uint8 else a.view(np.uint64)


def place(x, where):
    return dev(x) if where == "device" else np.ascontiguousarray(x)


def karr(K):
    return np.array(K, dtype=np.uint64).reshape(-1, 5)


def vectors(t):
    """gpu_scalars() in each term position in turn, then (1, L - 1, ..), (k, k, ..), all zero and the other planted vectors."""
    return SL.each_position_vectors(t, S.gpu_scalars()) + SL.planted_vectors(t)


def a_vector(t):
    """The last of the list's random scalars in the last position, random scalars in the others."""
    return SL.each_position_vectors(t, S.gpu_scalars())[-1]


def point_batch(oracle, n, t, K):
    P = SL.point_rows(oracle, t)
    idx = np.arange(n) % len(P)
    return np.ascontiguousarray(P[idx]), SL.want_ed_folded(oracle, t, K)[idx]


def point_batch_bytes(oracle, n, t, K):
    wb, wok = SL.want_ed_folded_bytes(oracle, t, K)
    idx = np.arange(n) % len(wb)
    return wb[idx], wok[idx]


def wire_batch(oracle, n, t, K):
    E, _ = SL.encoding_rows(oracle, t)
    idx = np.arange(n) % len(E)
    want, wok = SL.want_wire_folded(oracle, t, K)
    return np.ascontiguousarray(E[idx]), want[idx], wok[idx]


def test_the_folded_reference_is_oracle_lincomb(oracle):
    """The cached composition the tests below compare with is tests/lincomb_rows.oracle_lincomb / tests/ris_lincomb_rows.
    oracle_ris_lincomb with the vector tiled into every row (one vector per term count; CPU only)."""
    for t in (2, 5):
        K = vectors(t)[3][1]
        assert oracle.ed_eq(SL.want_ed_folded(oracle, t, K), SL.want_ed(oracle, t, K)).all()
        (a, aok), (b, bok) = SL.want_wire_folded(oracle, t, K), SL.want_wire(oracle, t, K)
        assert np.array_equal(a, b) and np.array_equal(aok, bok)


# ------------------------------------------------------------------ sizes, terms, placements, scalar vectors
@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("t", TERMS)
@pytest.mark.parametrize("n", SIZES)
def test_ed_form_is_the_oracles_group_element(eng, oracle, n, t, where):
    """zc_ed_eq = 1 against the oracle and the bytes of zc_ed_compress identical, for every vector of the list."""
    for name, K in vectors(t):
        a, want = point_batch(oracle, n, t, K)
        got = eng.ed_lincomb_shared(place(a, where), karr(K))
        assert isinstance(got, np.ndarray) == (where == "host") and tuple(got.shape) == (n, 20)
        eq = host(eng.ed_eq(got, place(want, where)))
        assert eq.all(), (name, np.flatnonzero(eq == 0)[:8])
        gb, gok = eng.ed_compress(got)
        wb, wok = point_batch_bytes(oracle, n, t, K)
        assert np.array_equal(host(gb), wb) and np.array_equal(host(gok), wok), name


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("t", TERMS)
@pytest.mark.parametrize("n", SIZES)
def test_wire_form_gives_the_oracles_bytes_and_those_of_ris_lincomb(eng, oracle, n, t, where):
    for vi, (name, K) in enumerate(vectors(t)):
        a, want, wok = wire_batch(oracle, n, t, K)
        got, ok = eng.ris_lincomb_shared(place(a, where), karr(K))
        assert isinstance(got, np.ndarray) == (where == "host") and tuple(got.shape) == (n, 32) and tuple(ok.shape) == (n,)
        got, ok = host(got), host(ok)
        assert np.array_equal(ok, wok), (name, np.flatnonzero(ok != wok)[:8])
        assert np.array_equal(got, want), (name, np.flatnonzero((got != want).any(axis=1))[:8])
        if vi % 3 == 0 or name in dict(SL.planted_vectors(t)):
            rt, rok = eng.ris_lincomb(place(a, where), place(SL.tile(K, n), where))
            assert np.array_equal(got, host(rt)) and np.array_equal(ok, host(rok)), name
    assert n < 331 or (wok == 0).sum() >= 4


@pytest.mark.parametrize("t", TERMS)
def test_a_python_list_of_ints_is_the_same_vector(eng, oracle, t):
    name, K = a_vector(t)
    a, _ = point_batch(oracle, 65, t, K)
    ints = [sum(int(x) << (52 * i) for i, x in enumerate(k)) for k in K]
    assert np.array_equal(eng.ed_lincomb_shared(a, ints), eng.ed_lincomb_shared(a, karr(K)))


def test_one_term_gives_the_limbs_and_bytes_of_the_single_scalar_calls(eng, oracle):
    for k in S.gpu_scalars():
        a, _ = point_batch(oracle, 1000, 1, [k])
        e, _, _ = wire_batch(oracle, 1000, 1, [k])
        for where in ("device", "host"):
            got = host(eng.ed_lincomb_shared(place(a, where), karr([k])))
            assert np.array_equal(got, host(eng.ed_scalar_mul_shared(place(a[:, 0], where), np.array(k, dtype=np.uint64)))), k
            b, ok = eng.ris_lincomb_shared(place(e, where), karr([k]))
            wb, wok = eng.ris_mul_shared(place(e[:, 0], where), np.array(k, dtype=np.uint64))
            assert np.array_equal(host(b), host(wb)) and np.array_equal(host(ok), host(wok)), k


@pytest.mark.parametrize("t", TERMS)
def test_limbs_do_not_depend_on_placement_or_batch_size(eng, oracle, t):
    for name, K in vectors(t)[::7]:
        a, _ = point_batch(oracle, 1000, t, K)
        d1000, h1000 = host(eng.ed_lincomb_shared(dev(a), karr(K))), eng.ed_lincomb_shared(a, karr(K))
        d65, h65 = host(eng.ed_lincomb_shared(dev(a[:65]), karr(K))), eng.ed_lincomb_shared(a[:65], karr(K))
        assert np.array_equal(d1000, h1000) and np.array_equal(d65, h65) and np.array_equal(d65, d1000[:65]), name
        assert (d1000 <= (1 << 52) - 1).all()


@pytest.mark.parametrize("t", [2, 8])
def test_planted_rows(eng, oracle, t):
    """P1 = -P0 with k0 = k1: the identity, as 32 zero bytes with ok = 1 in the wire form; P1 = P0: (2 k) P0; every point the
    identity: the identity under every vector; one zero scalar among non-zero ones is in the vector list of the tests above."""
    by_name = dict(SL.planted_vectors(t))
    K = by_name["(k, k, 0..)"]
    a, _ = point_batch(oracle, 331, t, K)
    got = host(eng.ed_lincomb_shared(dev(a), karr(K)))
    ident = np.tile(np.array(V.IDENT_ROW, dtype=np.uint64), (331, 1))
    assert oracle.ed_eq(got, ident)[list(SL.NEG_ROWS) + list(SL.IDENT_ROWS)].all()
    k2 = pm.limbs(2 * sum(int(x) << (52 * i) for i, x in enumerate(K[0])))
    dbl = eng.ed_scalar_mul_shared(np.ascontiguousarray(a[list(SL.SAME_ROWS), 0]), np.array(k2, dtype=np.uint64))
    assert oracle.ed_eq(got[list(SL.SAME_ROWS)], dbl).all()
    e, _, _ = wire_batch(oracle, 331, t, K)
    b, ok = [host(x) for x in eng.ris_lincomb_shared(dev(e), karr(K))]
    assert not b[list(SL.NEG_ROWS) + list(SL.IDENT_ROWS)].any() and ok[list(SL.NEG_ROWS) + list(SL.IDENT_ROWS)].all()
    for name, K in SL.planted_vectors(t):
        assert oracle.ed_eq(host(eng.ed_lincomb_shared(dev(a[list(SL.IDENT_ROWS)]), karr(K))), ident[:4]).all(), name


# ------------------------------------------------------------------ framed buffers
def raw(e, name, *args):
    """name(ctx, pointers and sizes..., n): integers below 64 are sizes, other integers pointers, None is NULL."""
    from dusk_zerocaf_amd import _lib
    conv = [None if a is None else (C.c_size_t(a) if a < 64 else C.c_void_p(a)) for a in args[:-1]]
    _lib.check(getattr(e.lib, name)(e.ctx, *conv, args[-1]), name, e.lib)


def _framed_call(e, backend, fn):
    import torch
    if backend == "torch":
        e._follow_torch_stream(torch.empty(1, dtype=torch.uint8, device="cuda"))

    def call(ip, op):
        fn(ip, op)
        torch.cuda.synchronize()
        e.synchronize()
    return call


@pytest.mark.parametrize("backend", ["torch", "numpy"])
@pytest.mark.parametrize("t", [1, 3, 8])
def test_framed_buffers_ed_form(eng, oracle, backend, t):
    """n = 300: frames and inputs as they were under zero and hostile fills, rows on a 16-byte boundary and 8 bytes off one; the
    outputs are the same under all of them; for one term in place (out == points) the same limbs again."""
    n = 300
    name, K = a_vector(t)
    k = karr(K)
    a, want = point_batch(oracle, n, t, K)
    a = a.reshape(n, 20 * t)
    frames = FB.hostile_frame_rows("pt*%d" % t if t > 1 else "pt", oracle)
    call = _framed_call(eng, backend, lambda ip, op: raw(eng, ED, ip[0], k.ctypes.data, t, op[0], n))
    got = {}
    for fill in (FB.ZERO, FB.HOSTILE):
        for shift in (0, 8):
            got[fill, shift] = FB.run_framed(call, [("points", a, frames)], [("out", n, 20, np.uint64)], backend=backend, fill=fill, in_shifts=[shift], out_shifts=[shift])
    first = got[FB.ZERO, 0]
    assert oracle.ed_eq(first[0], want).all()
    for key, res in got.items():
        FB.same_outputs(["out"], first, res, "%s, %s" % (ED, key))
    if t == 1:
        res = FB.run_framed(call, [("points", a, frames)], [("out", n, 20, np.uint64)], backend=backend, fill=FB.HOSTILE, in_shifts=[8], alias={0: 0})
        FB.same_outputs(["out"], first, res, "%s in place" % ED)


@pytest.mark.parametrize("backend", ["torch", "numpy"])
@pytest.mark.parametrize("t", [1, 3, 8])
def test_framed_buffers_wire_form(eng, oracle, backend, t):
    """The same for the wire form, with ok and with ok = NULL."""
    n = 300
    name, K = a_vector(t)
    k = karr(K)
    a, want, wok = wire_batch(oracle, n, t, K)
    a = a.reshape(n, 32 * t)
    frames = FB.hostile_frame_rows("enc32*%d" % t if t > 1 else "enc32", oracle)
    outs = [("out32", n, 32, np.uint8), ("ok", n, 0, np.uint8)]
    call = _framed_call(eng, backend, lambda ip, op: raw(eng, RIS, ip[0], k.ctypes.data, t, op[0], op[1], n))
    call_no_ok = _framed_call(eng, backend, lambda ip, op: raw(eng, RIS, ip[0], k.ctypes.data, t, op[0], None, n))
    got = {}
    for fill in (FB.ZERO, FB.HOSTILE):
        for shift in (0, 8):
            got[fill, shift] = FB.run_framed(call, [("in32", a, frames)], outs, backend=backend, fill=fill, in_shifts=[shift], out_shifts=[shift, shift])
    first = got[FB.ZERO, 0]
    assert np.array_equal(first[0], want) and np.array_equal(first[1], wok)
    for key, res in got.items():
        FB.same_outputs(["out32", "ok"], first, res, "%s, %s" % (RIS, key))
    res = FB.run_framed(call_no_ok, [("in32", a, frames)], outs[:1], backend=backend, fill=FB.HOSTILE, in_shifts=[8], out_shifts=[8])
    FB.same_outputs(["out32"], first[:1], res, "%s with ok = NULL" % RIS)


# ------------------------------------------------------------------ the caller's k
@pytest.mark.parametrize("t", [2, 8])
def test_k_may_be_overwritten_as_soon_as_the_call_returns(eng, oracle, t):
    """Device arrays, the call, the caller's words overwritten at once, then the synchronisation: the results are those of the
    original vector."""
    import torch
    n = 1000
    name, K = a_vector(t)
    a, want = point_batch(oracle, n, t, K)
    k = karr(K)
    p, out = dev(a), torch.empty((n, 20), dtype=torch.int64, device="cuda")
    eng._follow_torch_stream(p)
    raw(eng, ED, p.data_ptr(), k.ctypes.data, t, out.data_ptr(), n)
    k[:] = np.uint64((1 << 52) - 1)
    torch.cuda.synchronize()
    assert oracle.ed_eq(host(out), want).all()
    e, want, wok = wire_batch(oracle, n, t, K)
    k = karr(K)
    d, out, ok = dev(e), torch.empty((n, 32), dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    raw(eng, RIS, d.data_ptr(), k.ctypes.data, t, out.data_ptr(), ok.data_ptr(), n)
    k[:] = np.uint64((1 << 52) - 1)
    torch.cuda.synchronize()
    assert np.array_equal(host(out), want) and np.array_equal(host(ok), wok)


# ------------------------------------------------------------------ ring queueing
@pytest.mark.parametrize("t", [2, 8])
@pytest.mark.parametrize("slots", [8, 1])
def test_a_shrunken_table_ring_gives_the_bytes_of_the_default_context(eng, oracle, slots, t):
    """ZC_RING_SLOTS = 8 and 1: the waves of a 1000-row launch really queue for their multi-unit slots."""
    n = 1000
    name, K = a_vector(t)
    a, _ = point_batch(oracle, n, t, K)
    e, _, _ = wire_batch(oracle, n, t, K)
    ref_ed = host(eng.ed_lincomb_shared(dev(a), karr(K)))
    ref_b, ref_ok = [host(x) for x in eng.ris_lincomb_shared(dev(e), karr(K))]
    with V.tuned(ZC_RING_SLOTS=slots) as te:
        assert np.array_equal(host(te.ed_lincomb_shared(dev(a), karr(K))), ref_ed)
        b, ok = te.ris_lincomb_shared(dev(e), karr(K))
        assert np.array_equal(host(b), ref_b) and np.array_equal(host(ok), ref_ok)
        assert np.array_equal(te.ed_lincomb_shared(a, karr(K)), ref_ed)


# ------------------------------------------------------------------ row isolation
@pytest.mark.parametrize("wave", [0, 1, 2])
def test_one_hostile_row_changes_no_other_row(eng, oracle, wave):
    """One hostile record (off the curve, Z = 0 by value, limbs of all ones; a junk encoding) in one term of one row among 129
    good rows, in each of the first three waves in turn: every other row's output equals the run without it."""
    n, t = 130, 3
    name, K = a_vector(t)
    a, want = point_batch(oracle, n, t, K)
    clean = host(eng.ed_lincomb_shared(dev(a), karr(K)))
    assert oracle.ed_eq(clean, want).all()
    pats = dict(H.point_patterns(a[1, 0]))
    z0 = next(w for nm, w in pats.items() if nm.startswith("Z = ") and H.zero_by_value(w[10:15]) and any(w[:10]))
    at = 64 * wave + (1, 0, 1)[wave]                                            # row 129 is the third wave's last
    for j, w in enumerate((pats["off the curve"], z0, pats["every word all ones"])):
        b = a.copy()
        b[at, j] = np.array(w, dtype=np.uint64)
        got = host(eng.ed_lincomb_shared(dev(b), karr(K)))
        H.assert_others_unchanged(clean, got, [at], ED)
        assert np.array_equal(got, eng.ed_lincomb_shared(b, karr(K)))             # the hostile row's own limbs: the same on every path
    e, wantb, wok = wire_batch(oracle, n, t, K)
    cb, cok = [host(x) for x in eng.ris_lincomb_shared(dev(e), karr(K))]
    rng = np.random.default_rng(SL.SEED + wave)
    for j, junk in enumerate([b for _, b in H.undecodable(oracle.ris_decompress)][:2] + [rng.integers(0, 256, 32, dtype=np.uint8) | 0x80]):
        f = e.copy()
        f[at, j % t] = junk
        gb, gok = [host(x) for x in eng.ris_lincomb_shared(dev(f), karr(K))]
        H.assert_others_unchanged(cb, gb, [at], RIS)
        H.assert_others_unchanged(cok.reshape(n, 1), gok.reshape(n, 1), [at], RIS)
        assert gok[at] == 0 and not gb[at].any()


# ------------------------------------------------------------------ argument checks
def test_no_rows_mixed_memory_and_a_device_k(eng):
    import torch
    t = 2
    k = karr([pm.limbs(1), pm.limbs(pm.L - 1)])
    p, out = dev(np.zeros((4, t * 20), dtype=np.uint64)), torch.full((4, 20), 0x6E, dtype=torch.int64, device="cuda")
    enc, out32, ok = dev(np.zeros((4, t * 32), dtype=np.uint8)), torch.full((4, 32), 0xEE, dtype=torch.uint8, device="cuda"), torch.full((4,), 0xEE, dtype=torch.uint8, device="cuda")
    raw(eng, ED, p.data_ptr(), k.ctypes.data, t, out.data_ptr(), 0)
    raw(eng, RIS, enc.data_ptr(), k.ctypes.data, t, out32.data_ptr(), ok.data_ptr(), 0)
    torch.cuda.synchronize()
    assert (host(out) == 0x6E).all() and (host(out32) == 0xEE).all() and (host(ok) == 0xEE).all()
    assert eng.ed_lincomb_shared(np.zeros((0, t, 20), dtype=np.uint64), k).shape == (0, 20)
    hp, hout = np.zeros((4, t * 20), dtype=np.uint64), np.zeros((4, 20), dtype=np.uint64)
    henc, hout32 = np.zeros((4, t * 32), dtype=np.uint8), np.zeros((4, 32), dtype=np.uint8)
    v = lambda x: C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data)
    lib = eng.lib
    assert lib.zc_ed_lincomb_shared(eng.ctx, v(p), v(k), t, v(hout), 4) == ZC_ERR_MIXED_MEM
    assert lib.zc_ed_lincomb_shared(eng.ctx, v(hp), v(k), t, v(out), 4) == ZC_ERR_MIXED_MEM
    assert lib.zc_ris_lincomb_shared(eng.ctx, v(enc), v(k), t, v(hout32), None, 4) == ZC_ERR_MIXED_MEM
    assert lib.zc_ris_lincomb_shared(eng.ctx, v(henc), v(k), t, v(hout32), v(ok), 4) == ZC_ERR_MIXED_MEM
    dk = dev(k)
    assert lib.zc_ed_lincomb_shared(eng.ctx, v(p), v(dk), t, v(out), 4) == ZC_ERR_BAD_ARG
    assert lib.zc_last_error().decode() == "k must be host memory"
    assert lib.zc_ris_lincomb_shared(eng.ctx, v(henc), v(dk), t, v(hout32), None, 4) == ZC_ERR_BAD_ARG
    assert lib.zc_last_error().decode() == "k must be host memory"
    assert lib.zc_ed_lincomb_shared(eng.ctx, v(p), v(k), 9, v(out), 4) == ZC_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert (host(out) == 0x6E).all() and not hout.any() and not hout32.any()
