"""GPU tier: zc_sc_from_bytes_wide / zc_sc_from_bytes_mod_order, zc_sc_muladd and zc_sc_invert through the C ABI, every row
against Python integers (tests/scalar_ext_rows.py; none of the four is in the reference).  Host arrays and device tensors, byte
inputs from an odd address, outputs aliasing inputs, every launch form of the shared inversions, rows that are zero by value
planted at the first, middle and last position of a chunk, and a Schnorr sign / verify loop that never leaves the device."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from oracle import pymodel as pm
from tests import hostile_rows as H
from tests import scalar_ext_rows as S
from tests import vectors as V

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 257, 4099]
CHUNKS = [2, 3, 16, 64]
ONE = np.array([1, 0, 0, 0, 0], dtype=np.uint64)


@pytest.fixture(scope="module")
def eng():
    import dusk_zerocaf_amd as z
    e = z.Engine()
    yield e
    e.close()


def eq(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def dev(x):
    import torch
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x if x.dtype == np.uint8 else x.view(np.int64)).cuda()


def host(t):
    a = t.cpu().numpy()
    return a if a.dtype == np.uint8 else a.view(np.uint64)


def odd_address(t):
    """The same device rows starting one byte into an allocation."""
    import torch
    flat = torch.empty(t.numel() + 1, dtype=torch.uint8, device="cuda")
    v = flat[1:].view(t.shape)
    assert v.data_ptr() % 2 == 1 and v.is_contiguous()
    v.copy_(t)
    return v


@pytest.fixture(scope="module")
def big():
    """2^18 + 5 canonical non-zero scalars and their inverses, computed once; the launch-form tests take prefixes."""
    n = (1 << 18) + 5
    a = V.rand_scalars_np(n, V.SEED + 0x5D00, bits=249)
    a[:7] = S.invert_edges()
    want, wok = S.invert_expected(a)
    assert wok.all()
    for x in (a, want, wok):
        x.setflags(write=False)
    return a, want, wok


# ------------------------------------------------------------------ element-wise kernels
@pytest.mark.parametrize("width", [64, 32])
@pytest.mark.parametrize("n", SIZES)
def test_reduction_of_arbitrary_bytes(eng, width, n):
    fn = eng.sc_from_bytes_wide if width == 64 else eng.sc_from_bytes_mod_order
    edge = S.reduction_values(width, 0, 0)                                       # the edge values and every single-bit input
    rnd = S.reduction_values(width, n, V.SEED + 0x5D01 + n + width, bits=False)[-n:]
    vals = (edge + rnd)[:n] if n >= len(edge) else rnd
    if n < len(edge):                                                              # as many edges as fit, the rest over the sizes
        k = (n + 1) // 2
        start = (SIZES.index(n) * 7) % len(edge)
        vals[:k] = (edge + edge)[start:start + k]
    want = S.canon_rows(vals)
    b = S.to_bytes(vals, width)
    assert eq(fn(b), want)                                                         # host arrays
    buf = np.zeros(n * width + 1, dtype=np.uint8)
    buf[1:] = b.reshape(-1)
    assert eq(fn(buf[1:].reshape(n, width)), want)                                 # host arrays at an odd address
    d = dev(b)
    assert eq(host(fn(d)), want)                                                   # device tensors
    assert eq(host(fn(odd_address(d))), want)                                      # a device pointer one byte off: the unaligned loads
    if width == 32:
        assert eq(eng.sc_from_bytes_wide(np.concatenate([b, np.zeros_like(b)], axis=1)), want)


def test_reduction_edges_are_all_covered(eng):
    """Every edge value and single-bit input in one batch (the parametrised sizes below 4099 hold only a share of them)."""
    for width, fn in ((64, eng.sc_from_bytes_wide), (32, eng.sc_from_bytes_mod_order)):
        vals = S.reduction_values(width, 100, V.SEED + 0x5D02)
        assert eq(host(fn(dev(S.to_bytes(vals, width)))), S.canon_rows(vals))
    okb = S.to_bytes([S.L - 1, S.L, 2**256 - 1], 32)                               # where zc_sc_from_bytes refuses, this one reduces
    out, ok = eng.sc_from_bytes(okb)
    assert ok.tolist() == [1, 0, 0] and eq(eng.sc_from_bytes_mod_order(okb), S.canon_rows([S.L - 1, 0, 2**256 - 1]))


@pytest.mark.parametrize("n", SIZES)
def test_muladd(eng, n):
    fa, fb, fc = S.muladd_families(0, V.SEED + 0x5D03)
    a, b, c = (V.rand_scalars_np(n, V.SEED + 0x5D04 + n + j, bits=249) for j in range(3))
    k = min(len(fa), (n + 1) // 2)
    start = (SIZES.index(n) * 11) % len(fa)
    idx = [(start + j) % len(fa) for j in range(k)]
    pos = S.plant_among(a, fa[idx], V.SEED + 0x5D05 + n)
    b[pos], c[pos] = fb[idx], fc[idx]
    want = S.muladd_expected(a, b, c)
    assert eq(eng.sc_muladd(a, b, c), want)                                        # host arrays
    da, db, dc = dev(a), dev(b), dev(c)
    assert eq(host(eng.sc_muladd(da, db, dc)), want)                               # device tensors
    for which in range(3):                                                         # out aliasing a, b, c in turn
        ops = [da.clone(), db.clone(), dc.clone()]
        got = eng.sc_muladd(*ops, out=ops[which])
        assert got.data_ptr() == ops[which].data_ptr() and eq(host(got), want), which
        for j in range(3):
            assert j == which or eq(host(ops[j]), (a, b, c)[j])
    ha = a.copy()
    assert eq(eng.sc_muladd(ha, b, c, out=ha), want) and eq(ha, want)               # host, in place


def test_muladd_every_family_in_one_batch(eng):
    a, b, c = S.muladd_families(300, V.SEED + 0x5D06)
    want = S.muladd_expected(a, b, c)
    assert eq(host(eng.sc_muladd(dev(a), dev(b), dev(c))), want) and eq(eng.sc_muladd(a, b, c), want)


# ------------------------------------------------------------------ inversion: the launch forms
def _invert_raw(e, a_ptr, out_ptr, ok_ptr, n):
    from dusk_zerocaf_amd import _lib
    _lib.check(e.lib.zc_sc_invert(e.ctx, C.c_void_p(a_ptr), C.c_void_p(out_ptr), C.c_void_p(ok_ptr) if ok_ptr else None, n), "zc_sc_invert", e.lib)


def _all_forms(e, a, want, wok):
    """Host and device buffers, ok = NULL, in place (out == a) on the device: all must give `want`."""
    import torch
    n = len(a)
    out, ok = e.sc_invert(a)
    assert eq(out, want) and eq(ok, wok)
    d = dev(a)
    dout, dok = e.sc_invert(d)
    assert eq(host(dout), want) and eq(host(dok), wok)
    o2 = torch.full((n, 5), -1, dtype=torch.int64, device="cuda")
    e._follow_torch_stream(o2)
    _invert_raw(e, d.data_ptr(), o2.data_ptr(), 0, n)                              # ok = NULL
    assert eq(host(o2), want)
    h2 = np.zeros((n, 5), dtype=np.uint64)
    _invert_raw(e, a.ctypes.data, h2.ctypes.data, 0, n)                            # ok = NULL, host
    assert eq(h2, want)
    inplace = d.clone()
    okp = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    _invert_raw(e, inplace.data_ptr(), inplace.data_ptr(), okp.data_ptr(), n)      # out == a: one inversion per lane
    assert eq(host(inplace), want) and eq(host(okp), wok)
    torch.cuda.synchronize()


@pytest.mark.parametrize("c", CHUNKS)
def test_invert_shared_inversions_at_every_chunk(big, c):
    n = 128 * c + 7
    a, want, wok = (np.ascontiguousarray(x[:n]) for x in big)
    with V.tuned(ZC_INV_CHUNK=c) as te:
        _all_forms(te, a, want, wok)


def test_invert_default_context_one_per_lane(eng, big):
    a, want, wok = (np.ascontiguousarray(x[:257]) for x in big)
    _all_forms(eng, a, want, wok)


@pytest.mark.parametrize("n,c", [((1 << 17) + 3, 2), ((1 << 17) + 3, 3), ((1 << 18) + 5, 2)], ids=["2p17+3/2", "2p17+3/3", "2p18+5/2"])
def test_invert_large_launches(big, n, c):
    """The host takes k_sc_invert_chunked_lone while ceil(n / c) lanes leave at most one wave per SIMD (256 lanes per compute
    unit) and the column-ordered k_sc_invert_chunked beyond: on 256 compute units 2^17 + 3 rows at three per lane (43692
    lanes) are the former, 2^18 + 5 rows at two per lane (131075 lanes) the latter, 2^17 + 3 at two per lane (65538 lanes) sits
    just past the boundary.  Every row against pow(v, -1, L)."""
    a, want, wok = (np.ascontiguousarray(x[:n]) for x in big)
    with V.tuned(ZC_INV_CHUNK=c) as te:
        d = dev(a)
        out, ok = te.sc_invert(d)
        assert eq(host(out), want) and eq(host(ok), wok)
        if n < 1 << 18:
            out, ok = te.sc_invert(a)                                              # host buffers: the staged path
            assert eq(out, want) and eq(ok, wok)


@pytest.mark.parametrize("c", CHUNKS)
def test_rows_that_are_zero_by_value_change_no_other_row(big, c):
    """0, L, 2L, 255L, 2047L and a word of high bits only at the first, middle and last position of a chunk: out = 0, ok = 0
    for those, every other row identical to the same batch with the hostile rows replaced by 1 (and to pow(v, -1, L))."""
    n = 128 * c + 7
    pats = S.zero_patterns()
    hs = H.hostile_set(n, c)
    base, want0, _ = (np.array(x[:n]) for x in big)
    clean = base.copy()
    clean[hs] = ONE
    with V.tuned(ZC_INV_CHUNK=c) as te:
        ref = te.sc_invert(clean)
        dref = te.sc_invert(dev(clean))
        assert eq(ref[0], host(dref[0])) and eq(ref[1], host(dref[1])) and ref[1].all()
        for turn in range(len(pats)):
            a = base.copy()
            H.plant(a, hs, pats, turn)
            want, wok = want0.copy(), np.ones(n, dtype=np.uint8)
            want[hs], wok[hs] = 0, 0
            for got in (te.sc_invert(a), tuple(host(x) for x in te.sc_invert(dev(a)))):
                assert eq(got[0], want) and eq(got[1], wok), (c, turn)
                H.assert_others_unchanged(ref, got, hs, "sc_invert c=%d turn=%d" % (c, turn))
    one = S.zero_patterns()
    with V.tuned(ZC_INV_CHUNK=c) as te:                                            # a batch of nothing but zeros by value
        z = np.array([w for _, w in one] * 3, dtype=np.uint64)
        out, ok = te.sc_invert(z)
        assert not out.any() and not ok.any()


def test_zero_by_value_in_the_one_per_lane_kernel(eng):
    z = np.array([w for _, w in S.zero_patterns()] + [list(ONE)], dtype=np.uint64)
    out, ok = eng.sc_invert(z)
    assert ok.tolist() == [0] * (len(z) - 1) + [1] and not out[:-1].any() and eq(out[-1], ONE)


# ------------------------------------------------------------------ what the library offered before
def test_agrees_with_pow_and_with_mul_then_add(eng):
    n = 4099
    a, b, c = (V.rand_scalars_np(n, V.SEED + 0x5D10 + j, bits=249) for j in range(3))
    a[:len(V.SC_EDGE)] = V.limbs_array(V.SC_EDGE)
    inv, ok = eng.sc_invert(a)
    e = np.tile(np.array(pm.limbs(pm.L - 2), dtype=np.uint64), (n, 1))
    assert eq(inv, eng.sc_pow(a, e)) and ok.sum() == n - 1 and ok[0] == 0          # 0^(L-2) = 0
    assert eq(eng.sc_muladd(a, b, c), eng.sc_add(eng.sc_mul(a, b), c))
    nz = ok == 1
    assert (eng.sc_mul(a[nz], inv[nz]) == ONE).all()


# ------------------------------------------------------------------ a signature scheme on the device
def test_schnorr_sign_and_verify_stay_on_the_device(eng):
    """R = r B, A = x B (zc_ris_mul_base_compress); c = H(R | A | i) mod L (zc_sc_from_bytes_wide, SHA-512 on the host);
    s = c x + r (zc_sc_muladd); s B - c A (zc_ris_lincomb) is R byte for byte, ok = 1 on every row -- and with one bit of s
    flipped in a few rows, exactly those rows differ."""
    import torch
    n = 257
    r, x = dev(V.rand_scalars_np(n, V.SEED + 0x5D20, bits=249)), dev(V.rand_scalars_np(n, V.SEED + 0x5D21, bits=249))
    R, A = eng.ris_mul_base_compress(r), eng.ris_mul_base_compress(x)
    Rh, Ah = host(R), host(A)
    digest = np.frombuffer(b"".join(hashlib.sha512(Rh[i].tobytes() + Ah[i].tobytes() + i.to_bytes(8, "little")).digest() for i in range(n)),
                           dtype=np.uint8).reshape(n, 64)
    c = eng.sc_from_bytes_wide(dev(digest))
    assert eq(host(c), S.canon_rows([int.from_bytes(digest[i].tobytes(), "little") for i in range(n)]))
    s = eng.sc_muladd(c, x, r)
    assert eq(host(s), S.muladd_expected(host(c), host(x), host(r)))
    minus_c = eng.sc_neg(c)
    got, ok = eng.ris_lincomb(A.view(n, 1, 32), minus_c.view(n, 1, 5), base_scalars=s)
    assert eq(host(got), Rh) and host(ok).all() and isinstance(got, torch.Tensor)
    forged = [0, 5, 128, n - 1]
    sh = host(s).copy()
    for j, i in enumerate(forged):
        sh[i, j % 4] ^= np.uint64(1 << (3 + 11 * j))
    got, ok = eng.ris_lincomb(A.view(n, 1, 32), minus_c.view(n, 1, 5), base_scalars=dev(sh))
    differs = (host(got) != Rh).any(axis=1)
    assert np.flatnonzero(differs).tolist() == forged and host(ok).all()
