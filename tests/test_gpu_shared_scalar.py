"""GPU tier: zc_ed_scalar_mul_shared and zc_ris_mul_shared through the C ABI against the oracle (zc_ref) and against the calls
they replace with the scalar in every row.  Host arrays and device tensors, batch sizes on both sides of a wave and of a
workgroup with a ragged tail, undecodable rows in every wire-format batch (a whole wave of them too), framed buffers (nothing
outside rows 0 .. n-1 changes, inputs unchanged, arrays 8 bytes off a 16-byte boundary, in place, ok = NULL), the caller's k
overwritten right after the call, shrunken table rings, one hostile row among good ones, and the argument checks.  The rows
come from pools of at most 331 distinct rows (tests/shared_scalar_rows.py), repeated for longer batches."""
import ctypes as C

import numpy as np
import pytest

from oracle import pymodel as pm
from tests import framed_buffers as FB
from tests import hostile_rows as H
from tests import shared_scalar_rows as S
from tests import vectors as V

pytestmark = pytest.mark.gpu

ED, RIS = "zc_ed_scalar_mul_shared", "zc_ris_mul_shared"
SIZES = [1, 63, 65, 255, 257, 300, 1000]
SCALARS = S.gpu_scalars()
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


def karr(k):
    return np.array(k, dtype=np.uint64)


def point_batch(oracle, n, k):
    """n rows of the pool in turn and the oracle's k * P for them."""
    rows, _ = S.point_pool(oracle)
    idx = np.arange(n) % len(rows)
    return rows[idx], S.want_ed(oracle, rows, k)[idx]


def planted_rows(n):
    """Where a wire-format batch of n rows holds undecodable rows: every seventh row from row 3, and the whole second wave."""
    at = set(range(3, n, 7))
    if n >= 128:
        at |= set(range(64, 128))
    return sorted(at)


def wire_batch(oracle, n, k):
    """n rows of the encoding pool in turn with undecodable rows planted, and the oracle's (bytes, ok) for them."""
    enc = S.encoding_pool(oracle)
    idx = np.arange(n) % len(enc)
    want, wok = S.want_wire(oracle, enc, k)
    a, w, o = enc[idx].copy(), want[idx].copy(), wok[idx].copy()
    bad = [b for _, b in H.undecodable(oracle.ris_decompress)]
    for j, i in enumerate(planted_rows(n)):
        a[i], w[i], o[i] = bad[j % len(bad)], 0, 0
    return a, w, o


# ------------------------------------------------------------------ sizes, placements, scalars
@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("n", SIZES)
def test_ed_form_is_the_oracles_group_element(eng, oracle, n, where):
    """zc_ed_eq = 1 against the oracle and the bytes of zc_ed_compress identical, for every scalar of the list."""
    for k in SCALARS:
        a, want = point_batch(oracle, n, k)
        got = eng.ed_scalar_mul_shared(place(a, where), karr(k))
        assert isinstance(got, np.ndarray) == (where == "host") and tuple(got.shape) == (n, 20)
        eq = host(eng.ed_eq(got, place(want, where)))
        assert eq.all(), (k, np.flatnonzero(eq == 0)[:8])
        (gb, gok), (wb, wok) = eng.ed_compress(got), eng.ed_compress(place(want, where))
        assert np.array_equal(host(gb), host(wb)) and np.array_equal(host(gok), host(wok)), k
        assert np.array_equal(host(gb), oracle.ed_compress(want)[0]), k


def test_ed_form_limbs_do_not_depend_on_placement_or_batch_size(eng, oracle):
    for k in SCALARS:
        a, _ = point_batch(oracle, 1000, k)
        d1000, h1000 = host(eng.ed_scalar_mul_shared(dev(a), karr(k))), eng.ed_scalar_mul_shared(a, karr(k))
        d300, h300 = host(eng.ed_scalar_mul_shared(dev(a[:300]), karr(k))), eng.ed_scalar_mul_shared(a[:300], karr(k))
        assert np.array_equal(d1000, h1000) and np.array_equal(d300, h300) and np.array_equal(d300, d1000[:300]), k
        assert (d1000 <= (1 << 52) - 1).all()


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("n", SIZES)
def test_wire_form_gives_the_oracles_bytes_and_those_of_roundtrip_mul(eng, oracle, n, where):
    for k in SCALARS:
        a, want, wok = wire_batch(oracle, n, k)
        got, ok = eng.ris_mul_shared(place(a, where), karr(k))
        assert isinstance(got, np.ndarray) == (where == "host") and tuple(got.shape) == (n, 32) and tuple(ok.shape) == (n,)
        got, ok = host(got), host(ok)
        assert np.array_equal(ok, wok), (k, np.flatnonzero(ok != wok)[:8])
        assert np.array_equal(got, want), (k, np.flatnonzero((got != want).any(axis=1))[:8])
        rt, rok = eng.ris_roundtrip_mul(place(a, where), place(S.tile(k, n), where))
        assert np.array_equal(got, host(rt)) and np.array_equal(ok, host(rok)), k
    assert n < 128 or (wok[64:128] == 0).all()                                   # a whole wave of undecodable rows


def test_a_product_that_is_the_identity_leaves_as_zero_bytes_with_ok_set(eng, oracle):
    a, _, _ = wire_batch(oracle, 300, SCALARS[0])
    dec = oracle.ris_decompress(a)[1]
    for k in (pm.limbs(0), pm.limbs(pm.L)):
        got, ok = eng.ris_mul_shared(dev(a), karr(k))
        assert not host(got).any() and np.array_equal(host(ok), dec)
    got, ok = eng.ris_mul_shared(dev(a), 1)                                       # a Python int for k
    assert np.array_equal(host(got)[dec == 1], a[dec == 1])


# ------------------------------------------------------------------ framed buffers
def raw(e, name, *args):
    """name(ctx, pointers..., n): the pointers as integers, or None for NULL."""
    from dusk_zerocaf_amd import _lib
    ptrs = [None if a is None else C.c_void_p(a) for a in args[:-1]]
    _lib.check(getattr(e.lib, name)(e.ctx, *ptrs, args[-1]), name, e.lib)


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
def test_framed_buffers_ed_form(eng, oracle, backend):
    """n = 300: frames and inputs as they were under zero and hostile fills, rows on a 16-byte boundary and 8 bytes off one; the
    outputs are the same under all of them; in place (out == p) the same limbs again."""
    n, k = 300, karr(SCALARS[-1])
    a, want = point_batch(oracle, n, SCALARS[-1])
    frames = FB.hostile_frame_rows("pt", oracle)
    call = _framed_call(eng, backend, lambda ip, op: raw(eng, ED, ip[0], k.ctypes.data, op[0], n))
    got = {}
    for fill in (FB.ZERO, FB.HOSTILE):
        for shift in (0, 8):
            got[fill, shift] = FB.run_framed(call, [("p", a, frames)], [("out", n, 20, np.uint64)], backend=backend, fill=fill, in_shifts=[shift], out_shifts=[shift])
    first = got[FB.ZERO, 0]
    assert oracle.ed_eq(first[0], want).all()
    for key, res in got.items():
        FB.same_outputs(["out"], first, res, "%s, %s" % (ED, key))
    for shift in (0, 8):
        res = FB.run_framed(call, [("p", a, frames)], [("out", n, 20, np.uint64)], backend=backend, fill=FB.HOSTILE, in_shifts=[shift], alias={0: 0})
        FB.same_outputs(["out"], first, res, "%s in place, rows %d bytes off" % (ED, shift))


@pytest.mark.parametrize("backend", ["torch", "numpy"])
def test_framed_buffers_wire_form(eng, oracle, backend):
    """The same for the wire form, with ok, with ok = NULL and with out32 == in32."""
    n, k = 300, karr(SCALARS[-1])
    a, want, wok = wire_batch(oracle, n, SCALARS[-1])
    frames = FB.hostile_frame_rows("enc32", oracle)
    outs = [("out32", n, 32, np.uint8), ("ok", n, 0, np.uint8)]
    call = _framed_call(eng, backend, lambda ip, op: raw(eng, RIS, ip[0], k.ctypes.data, op[0], op[1], n))
    call_no_ok = _framed_call(eng, backend, lambda ip, op: raw(eng, RIS, ip[0], k.ctypes.data, op[0], None, n))
    got = {}
    for fill in (FB.ZERO, FB.HOSTILE):
        for shift in (0, 8):
            got[fill, shift] = FB.run_framed(call, [("in32", a, frames)], outs, backend=backend, fill=fill, in_shifts=[shift], out_shifts=[shift, shift])
    first = got[FB.ZERO, 0]
    assert np.array_equal(first[0], want) and np.array_equal(first[1], wok)
    for key, res in got.items():
        FB.same_outputs(["out32", "ok"], first, res, "%s, %s" % (RIS, key))
    for shift in (0, 8):
        res = FB.run_framed(call_no_ok, [("in32", a, frames)], outs[:1], backend=backend, fill=FB.HOSTILE, in_shifts=[shift], out_shifts=[shift])
        FB.same_outputs(["out32"], first[:1], res, "%s with ok = NULL" % RIS)
        res = FB.run_framed(call, [("in32", a, frames)], outs, backend=backend, fill=FB.HOSTILE, in_shifts=[shift], out_shifts=[0, shift], alias={0: 0})
        FB.same_outputs(["out32", "ok"], first, res, "%s in place, rows %d bytes off" % (RIS, shift))


# ------------------------------------------------------------------ the caller's k
def test_k_may_be_overwritten_as_soon_as_the_call_returns(eng, oracle):
    """Device arrays, the call, the caller's five words overwritten at once, then the synchronisation: the results are those of
    the original k."""
    import torch
    n = 1000
    for name in (ED, RIS):
        k0 = SCALARS[-2]
        k = karr(k0)
        if name == ED:
            a, want = point_batch(oracle, n, k0)
            p, out = dev(a), torch.empty((n, 20), dtype=torch.int64, device="cuda")
            eng._follow_torch_stream(p)
            raw(eng, ED, p.data_ptr(), k.ctypes.data, out.data_ptr(), n)
            k[:] = np.uint64((1 << 52) - 1)
            torch.cuda.synchronize()
            assert oracle.ed_eq(host(out), want).all()
        else:
            a, want, wok = wire_batch(oracle, n, k0)
            e, out, ok = dev(a), torch.empty((n, 32), dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
            eng._follow_torch_stream(e)
            raw(eng, RIS, e.data_ptr(), k.ctypes.data, out.data_ptr(), ok.data_ptr(), n)
            k[:] = np.uint64((1 << 52) - 1)
            torch.cuda.synchronize()
            assert np.array_equal(host(out), want) and np.array_equal(host(ok), wok)


# ------------------------------------------------------------------ ring queueing
@pytest.mark.parametrize("slots", [8, 1])
def test_a_shrunken_table_ring_gives_the_bytes_of_the_default_context(eng, oracle, slots):
    n, k = 1000, SCALARS[-1]
    a, _ = point_batch(oracle, n, k)
    e, _, _ = wire_batch(oracle, n, k)
    ref_ed = host(eng.ed_scalar_mul_shared(dev(a), karr(k)))
    ref_b, ref_ok = [host(x) for x in eng.ris_mul_shared(dev(e), karr(k))]
    with V.tuned(ZC_RING_SLOTS=slots) as te:
        assert np.array_equal(host(te.ed_scalar_mul_shared(dev(a), karr(k))), ref_ed)
        b, ok = te.ris_mul_shared(dev(e), karr(k))
        assert np.array_equal(host(b), ref_b) and np.array_equal(host(ok), ref_ok)
        assert np.array_equal(te.ed_scalar_mul_shared(a, karr(k)), ref_ed)


# ------------------------------------------------------------------ row isolation
@pytest.mark.parametrize("wave", [0, 1, 2])
def test_one_hostile_row_changes_no_other_row(eng, oracle, wave):
    """One hostile record (off the curve, Z = 0 by value, limbs of all ones) among 129 good rows, in each of the first three
    waves in turn: every other row's output equals the run without it."""
    n, k = 130, SCALARS[-1]
    a, want = point_batch(oracle, n, k)
    clean = host(eng.ed_scalar_mul_shared(dev(a), karr(k)))
    assert oracle.ed_eq(clean, want).all()
    pats = dict(H.point_patterns(a[1]))
    z0 = next(w for nm, w in pats.items() if nm.startswith("Z = ") and H.zero_by_value(w[10:15]) and any(w[:10]))
    at = 64 * wave + (1, 0, 1)[wave]                                            # row 129 is the third wave's last
    for w in (pats["off the curve"], z0, pats["every word all ones"]):
        b = a.copy()
        b[at] = np.array(w, dtype=np.uint64)
        got = host(eng.ed_scalar_mul_shared(dev(b), karr(k)))
        H.assert_others_unchanged(clean, got, [at], ED)
        assert np.array_equal(got, eng.ed_scalar_mul_shared(b, karr(k)))          # the hostile row's own limbs: the same on every path


# ------------------------------------------------------------------ argument checks
def test_no_rows_mixed_memory_and_a_device_k(eng):
    import torch
    k = karr(SCALARS[1])
    p, out = dev(np.zeros((4, 20), dtype=np.uint64)), torch.full((4, 20), 0x6E, dtype=torch.int64, device="cuda")
    enc, out32, ok = dev(np.zeros((4, 32), dtype=np.uint8)), torch.full((4, 32), 0xEE, dtype=torch.uint8, device="cuda"), torch.full((4,), 0xEE, dtype=torch.uint8, device="cuda")
    raw(eng, ED, p.data_ptr(), k.ctypes.data, out.data_ptr(), 0)
    raw(eng, RIS, enc.data_ptr(), k.ctypes.data, out32.data_ptr(), ok.data_ptr(), 0)
    torch.cuda.synchronize()
    assert (host(out) == 0x6E).all() and (host(out32) == 0xEE).all() and (host(ok) == 0xEE).all()
    assert eng.ed_scalar_mul_shared(np.zeros((0, 20), dtype=np.uint64), k).shape == (0, 20)
    hp, hout = np.zeros((4, 20), dtype=np.uint64), np.zeros((4, 20), dtype=np.uint64)
    henc, hout32 = np.zeros((4, 32), dtype=np.uint8), np.zeros((4, 32), dtype=np.uint8)
    v = lambda x: C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data)
    lib = eng.lib
    assert lib.zc_ed_scalar_mul_shared(eng.ctx, v(p), v(k), v(hout), 4) == ZC_ERR_MIXED_MEM
    assert lib.zc_ed_scalar_mul_shared(eng.ctx, v(hp), v(k), v(out), 4) == ZC_ERR_MIXED_MEM
    assert lib.zc_ris_mul_shared(eng.ctx, v(enc), v(k), v(hout32), None, 4) == ZC_ERR_MIXED_MEM
    assert lib.zc_ris_mul_shared(eng.ctx, v(henc), v(k), v(hout32), v(ok), 4) == ZC_ERR_MIXED_MEM
    dk = dev(k.reshape(1, 5))
    assert lib.zc_ed_scalar_mul_shared(eng.ctx, v(p), v(dk), v(out), 4) == ZC_ERR_BAD_ARG
    assert lib.zc_last_error().decode() == "k must be host memory"
    assert lib.zc_ris_mul_shared(eng.ctx, v(henc), v(dk), v(hout32), None, 4) == ZC_ERR_BAD_ARG
    assert lib.zc_last_error().decode() == "k must be host memory"
    torch.cuda.synchronize()
    assert (host(out) == 0x6E).all() and not hout.any() and not hout32.any()
