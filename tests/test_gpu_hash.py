"""GPU tier: zc_sha512_rows, zc_sc_from_sha512 and zc_ris_from_sha512 through the C ABI.  Digests against hashlib, scalars
against Python integers, points against the oracle's from_uniform_bytes of the digest (tests/hash_rows.py).  Host arrays and
device tensors, parts at odd device addresses, the byte form forced on aligned inputs (test-hooks library), host batches cut
into chunks, the two fused calls against the calls they fuse, framed buffers, and a Schnorr sign / verify loop whose challenge
hash never leaves the device."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from tests import framed_buffers as FB
from tests import hash_rows as HR
from tests import scalar_ext_rows as S
from tests import vectors as V

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 257, 4099]
SHAPES = [(1,), (32, 32, 32), (111,), (112,), (127,), (128,), (129,), (5, 3, 120, 1), (240,), (1000,)]
PREFIX_LENS = [0, 6, 128, 256]
POINT_ROWS = 257            # batches up to here have every point checked against the oracle; larger ones a spread of rows (below)
_cache = {}


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


def rows_for(shape, n):
    """Seeded parts of `shape` for 4099 rows, made once and never written; a batch of n rows is their first n."""
    if shape not in _cache:
        parts = HR.random_parts(SIZES[-1], list(shape), V.SEED + 0x6A00 + sum(shape) + len(shape))
        for p in parts:
            p.setflags(write=False)
        _cache[shape] = parts
    return [p[:n].copy() for p in _cache[shape]]


def spread(n):
    """Rows of a large batch whose points go to the oracle (0.4 ms each): the first and last row, both sides of every wave
    and workgroup edge up to 512, and every 97th row."""
    return sorted({i for i in [0, 1, 62, 63, 64, 65, 127, 128, 255, 256, 257, 511, 512, n - 2, n - 1] + list(range(0, n, 97)) if 0 <= i < n})


def expected(parts, prefix):
    dig = HR.digests(parts, prefix)
    return dig, HR.scalars_of(dig)


# ------------------------------------------------------------------ digests, scalars, points
@pytest.mark.parametrize("plen", PREFIX_LENS)
@pytest.mark.parametrize("n", SIZES)
def test_digests_scalars_and_points(eng, oracle, n, plen):
    """Every part shape at this batch size and prefix length, as host arrays and as device tensors; (1000,) at n = 65 only.
    Digests and scalars: every row.  Points: every row against the oracle up to 257 rows; at 4099 rows the whole batch for
    (32, 32, 32), for the other shapes the rows of spread() against the oracle and the whole batch limb for limb against
    zc_ris_from_uniform_bytes of the digests just verified (the oracle takes 1.6 s per 4099 rows)."""
    prefix = HR.prefix_bytes(plen, plen)
    for shape in SHAPES:
        if shape == (1000,) and n != 65:
            continue
        parts = rows_for(shape, n)
        dig, sc = expected(parts, prefix)
        every = n <= POINT_ROWS or shape == (32, 32, 32)
        idx = list(range(n)) if every else spread(n)
        want_pts = oracle.ris_from_uniform_bytes(dig[idx])
        composed = None if every else eng.ris_from_uniform_bytes(dig)
        for kind in ("host", "device"):
            ins = parts if kind == "host" else [dev(p) for p in parts]
            out = lambda x: x if kind == "host" else host(x)
            assert eq(out(eng.sha512_rows(ins, prefix)), dig), (shape, kind)
            assert eq(out(eng.sc_from_sha512(ins, prefix)), sc), (shape, kind)
            pts = out(eng.ris_from_sha512(ins, prefix))
            assert eq(pts[idx], want_pts) and (every or eq(pts, composed)), (shape, kind)


# ------------------------------------------------------------------ launch forms and addresses
@pytest.mark.parametrize("shape,plen", [((32, 32, 32), 6), ((32, 32, 32), 8), ((128,), 0), ((5, 3, 120, 1), 128), ((240,), 256)])
def test_device_parts_at_an_odd_address(eng, oracle, shape, plen):
    n = 257
    prefix = HR.prefix_bytes(plen)
    parts = rows_for(shape, n)
    dig, sc = expected(parts, prefix)
    ins = [odd_address(dev(p)) for p in parts]
    assert eq(host(eng.sha512_rows(ins, prefix)), dig)
    assert eq(host(eng.sc_from_sha512(ins, prefix)), sc)
    assert eq(host(eng.ris_from_sha512(ins, prefix)), oracle.ris_from_uniform_bytes(dig))
    # the digests themselves written from an odd address on
    import torch
    flat = torch.full((n * 64 + 1,), 0xA5, dtype=torch.uint8, device="cuda")
    eng._follow_torch_stream(flat)
    k = len(ins)
    rc = eng.lib.zc_sha512_rows(eng.ctx, prefix if prefix else None, len(prefix), (C.c_void_p * k)(*[t.data_ptr() for t in ins]), (C.c_size_t * k)(*shape), k,
                                C.c_void_p(flat.data_ptr() + 1), n)
    assert rc == 0, eng.lib.zc_last_error()
    torch.cuda.synchronize()
    assert eq(flat[1:].cpu().numpy().reshape(n, 64), dig) and int(flat[0]) == 0xA5


@pytest.mark.parametrize("shape,plen", [((32, 32, 32), 8), ((128,), 0), ((8, 104), 128), ((240,), 256), ((1000,), 16)])
def test_forced_byte_form_equals_word_form_on_aligned_inputs(oracle, shape, plen):
    """The test-hooks library with and without ZC_TEST_HASH_READER=bytes: aligned device and host inputs, all three calls."""
    n = 257
    prefix = HR.prefix_bytes(plen)
    parts = rows_for(shape, n)
    dig, sc = expected(parts, prefix)
    pts = oracle.ris_from_uniform_bytes(dig)
    with V.tuned(hooks=True) as words, V.tuned(hooks=True, ZC_TEST_HASH_READER="bytes") as forced:
        ins = [dev(p) for p in parts]
        assert all(t.data_ptr() % 8 == 0 for t in ins)
        for e in (words, forced):
            assert eq(host(e.sha512_rows(ins, prefix)), dig) and eq(e.sha512_rows(parts, prefix), dig)
            assert eq(host(e.sc_from_sha512(ins, prefix)), sc) and eq(e.sc_from_sha512(parts, prefix), sc)
            assert eq(host(e.ris_from_sha512(ins, prefix)), pts) and eq(e.ris_from_sha512(parts, prefix), pts)


@pytest.mark.parametrize("chunks", [1, 3, 7])
def test_host_arrays_cut_into_chunks(chunks):
    n = 4099
    with V.tuned(ZC_HOST_CHUNKS=chunks) as e:
        for shape, plen in (((32, 32, 32), 6), ((8, 104), 8), ((5, 3, 120, 1), 0)):
            prefix = HR.prefix_bytes(plen)
            parts = rows_for(shape, n)
            dig, sc = expected(parts, prefix)
            assert eq(e.sha512_rows(parts, prefix), dig) and eq(e.sc_from_sha512(parts, prefix), sc)
            assert eq(e.ris_from_sha512(parts, prefix), e.ris_from_uniform_bytes(dig))


# ------------------------------------------------------------------ the calls they fuse
@pytest.mark.parametrize("kind", ["host", "device"])
def test_fused_calls_equal_their_compositions(eng, kind):
    n = 4099
    for shape, plen in (((32, 32, 32), 6), ((128,), 0), ((5, 3, 120, 1), 256), ((1,), 0)):
        prefix = HR.prefix_bytes(plen)
        parts = rows_for(shape, n)
        ins = parts if kind == "host" else [dev(p) for p in parts]
        out = lambda x: x if kind == "host" else host(x)
        dig = eng.sha512_rows(ins, prefix)
        assert eq(out(eng.sc_from_sha512(ins, prefix)), out(eng.sc_from_bytes_wide(dig)))
        assert eq(out(eng.ris_from_sha512(ins, prefix)), out(eng.ris_from_uniform_bytes(dig)))


# ------------------------------------------------------------------ bounds
CALLS = [("zc_sha512_rows", "out64", 64, np.uint8), ("zc_sc_from_sha512", "out", 5, np.uint64), ("zc_ris_from_sha512", "out", 20, np.uint64)]


@pytest.mark.parametrize("backend", ["numpy", "torch"])
@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("name,out_name,width,dtype", CALLS, ids=[c[0] for c in CALLS])
def test_framed_buffers(eng, oracle, backend, n, name, out_name, width, dtype):
    """Rows in the middle of larger allocations (the byte parts 3 bytes past a 16-byte boundary, the output 8): every byte
    outside rows 0 .. n-1 of the output and every input byte is unchanged, and what surrounds the parts does not reach the
    result."""
    import torch
    shape, prefix = (32, 32, 5), HR.prefix_bytes(6)
    parts = rows_for((32, 32, 32), n)[:2] + [np.ascontiguousarray(rows_for((5, 3, 120, 1), n)[0])]
    dig, sc = expected(parts, prefix)
    want = dig if width == 64 else sc if width == 5 else oracle.ris_from_uniform_bytes(dig)
    k = len(parts)
    runs = []
    for fill in (FB.ZERO, FB.HOSTILE):
        def call(ip, op):
            torch.cuda.synchronize()
            rc = getattr(eng.lib, name)(eng.ctx, prefix, len(prefix), (C.c_void_p * k)(*ip), (C.c_size_t * k)(*shape), k, C.c_void_p(op[0]), n)
            assert rc == 0, eng.lib.zc_last_error()
            torch.cuda.synchronize()
        inputs = [("parts[%d]" % j, p, np.full((3, p.shape[1]), 0xFF, dtype=np.uint8)) for j, p in enumerate(parts)]
        got = FB.run_framed(call, inputs, [(out_name, n, width, dtype)], backend=backend, fill=fill, in_shifts=[3] * k, out_shifts=[1 if width == 64 else 8])
        assert eq(got[0], want)
        runs.append(got)
    FB.same_outputs([out_name], runs[0], runs[1], name)


def test_placement_and_argument_errors(eng):
    """Host parts with a device output and the reverse are ZC_ERR_MIXED_MEM; n == 0 is ZC_OK and writes nothing; the limits
    are refused with a live context as with none."""
    import torch
    n = 64
    parts = rows_for((32, 32, 32), n)
    dparts = [dev(p) for p in parts]
    out, dout = np.full((n, 64), 0xA5, dtype=np.uint8), dev(np.full((n, 64), 0xA5, dtype=np.uint8))
    lens = (C.c_size_t * 3)(32, 32, 32)
    hp, dp = [p.ctypes.data for p in parts], [t.data_ptr() for t in dparts]
    call = lambda ptrs, o, rows=n, pl=0, nparts=3: eng.lib.zc_sha512_rows(eng.ctx, b"x" * pl if pl else None, pl, (C.c_void_p * 3)(*ptrs), lens, nparts, C.c_void_p(o), rows)
    ZC_ERR_BAD_ARG, ZC_ERR_MIXED_MEM = -1, -5
    assert call(hp, dout.data_ptr()) == ZC_ERR_MIXED_MEM and b"mixed" in eng.lib.zc_last_error()
    assert call(dp, out.ctypes.data) == ZC_ERR_MIXED_MEM and call([hp[0], dp[1], hp[2]], out.ctypes.data) == ZC_ERR_MIXED_MEM
    assert call(hp, out.ctypes.data, rows=0) == 0 and call(dp, dout.data_ptr(), rows=0) == 0
    assert call(hp, out.ctypes.data, pl=257) == ZC_ERR_BAD_ARG and call(hp, out.ctypes.data, nparts=0) == ZC_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert (out == 0xA5).all() and bool((dout == 0xA5).all())
    assert eq(eng.sha512_rows(parts), HR.digests(parts))                             # the context is as usable as before


# ------------------------------------------------------------------ a signature scheme on the device
def test_schnorr_loop_never_leaves_the_device(eng):
    """INTEGRATION.md section 4e with the challenge hashed on the device: R = r B, A = x B (zc_ris_mul_base_compress),
    c = SHA-512("domain" | R | A | m) mod L (zc_sc_from_sha512), s = c x + r (zc_sc_muladd).  Every row verifies through
    zc_ris_lincomb (s B - c A is R byte for byte), the batch through zc_ris_lincomb_sum with random weights, the challenges are
    the ones hashlib gives on the downloaded R, A, m -- and one flipped message byte makes exactly that row fail."""
    import torch
    n = 4099
    domain = b"domain"
    r, x = dev(V.rand_scalars_np(n, V.SEED + 0x6B00, bits=249)), dev(V.rand_scalars_np(n, V.SEED + 0x6B01, bits=249))
    m = dev(rows_for((32, 32, 32), n)[2])
    R, A = eng.ris_mul_base_compress(r), eng.ris_mul_base_compress(x)
    c = eng.sc_from_sha512([R, A, m], domain)
    assert isinstance(c, torch.Tensor) and c.is_cuda
    s = eng.sc_muladd(c, x, r)

    def verify(msg):
        ch = eng.sc_from_sha512([R, A, msg], domain)
        got, ok = eng.ris_lincomb(A.view(n, 1, 32), eng.sc_neg(ch).view(n, 1, 5), base_scalars=s)
        return ch, (host(got) == host(R)).all(axis=1) & (host(ok) == 1)
    ch, good = verify(m)
    assert good.all()
    Rh, Ah, mh = host(R), host(A), host(m)
    want = S.canon_rows([int.from_bytes(hashlib.sha512(domain + Rh[i].tobytes() + Ah[i].tobytes() + mh[i].tobytes()).digest(), "little") for i in range(n)])
    assert eq(host(c), want) and eq(host(ch), want)
    # the batch: sum_i z_i (s_i B - c_i A_i - R_i) = identity, z_i of 128 random bits
    z = V.rand_scalars_np(n, V.SEED + 0x6B02, bits=249)
    z[:, 2] &= np.uint64((1 << 24) - 1)
    z[:, 3:] = 0
    z = dev(z)
    enc = torch.stack([A, R], dim=1).contiguous()
    minus_one = dev(np.tile(np.array(S.canon_rows([S.L - 1])[0]), (n, 1)))
    ks = torch.stack([eng.sc_neg(c), minus_one], dim=1).contiguous()
    total, ok = eng.ris_lincomb_sum(enc, ks, base_scalars=s, weights=z)
    assert total == bytes(32) and host(ok).all()
    forged = mh.copy()
    forged[1234, 7] ^= 0x10
    _, still = verify(dev(forged))
    assert np.flatnonzero(~still).tolist() == [1234]
