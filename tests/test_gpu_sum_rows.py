"""GPU tier: the point sums (zc_ed_sum_rows, zc_ris_sum_rows) through the C ABI against tests/sum_rows.py: model_sum -- the
oracle's ed_add in the documented order -- limb for limb, and the oracle's decompress / add / ris_compress byte for byte.  Term
counts on both sides of every boundary of the plan (the serial limit, the first count with 2 parts, the largest parts one
workgroup finishes and the next, uneven slices), host arrays and device tensors, batch sizes on both sides of a wave and of a
workgroup, framed buffers, arrays 8 bytes off a 16-byte boundary, two calls in flight on two streams with the two-kernel form,
and the argument checks.  The model's answers are computed once per term count."""
import ctypes as C

import numpy as np
import pytest

from tests import framed_buffers as FB
from tests import hostile_rows as HR
from tests import sum_rows as SR

pytestmark = pytest.mark.gpu

ED, RIS = "zc_ed_sum_rows", "zc_ris_sum_rows"
ZC_ERR_BAD_ARG, ZC_ERR_MIXED_MEM = -1, -5
CASES = [(t, n) for t in SR.SHORT_TERMS for n in SR.SHORT_N] + [(t, n) for t in SR.LONG_TERMS for n in SR.LONG_N]


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


def err(e):
    return e.lib.zc_last_error().decode()


def v(x):
    return None if x is None else C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data)


# ------------------------------------------------------------------ term counts, sizes, placements
@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("terms,n", CASES)
def test_both_forms_are_the_models(eng, oracle, terms, n, where):
    pts = SR.points(oracle, n, terms)
    got = eng.ed_sum_rows(place(pts, where))
    assert isinstance(got, np.ndarray) == (where == "host") and tuple(got.shape) == (n, 20)
    want = SR.want_ed(oracle, n, terms)
    assert np.array_equal(host(got), want), np.flatnonzero((host(got) != want).any(axis=1))[:8]
    enc, _ = SR.encodings(oracle, n, terms)
    wb, wok = SR.want_wire(oracle, n, terms)
    out, ok = eng.ris_sum_rows(place(enc, where))
    assert isinstance(out, np.ndarray) == (where == "host") and tuple(out.shape) == (n, 32) and tuple(ok.shape) == (n,)
    assert np.array_equal(host(ok), wok) and np.array_equal(host(out), wb), np.flatnonzero((host(out) != wb).any(axis=1))[:8]


@pytest.mark.parametrize("terms", [3, 33, 4096, 8197])
def test_wire_form_is_zc_ris_compress_of_the_edwards_form_on_decoded_inputs(eng, oracle, terms):
    n = 3 if terms in SR.LONG_TERMS else 257
    enc, wok = SR.encodings(oracle, n, terms)
    d = dev(enc)
    pts, _ = eng.ris_decompress(d.reshape(n * terms, 32))
    comp = host(eng.ris_compress(eng.ed_sum_rows(pts.reshape(n, terms, 20))))
    comp[wok == 0] = 0
    assert np.array_equal(host(eng.ris_sum_rows(d)[0]), comp)


@pytest.mark.parametrize("terms", [2, 33, 8192])
def test_ok_may_be_null(eng, oracle, terms):
    n = 3 if terms in SR.LONG_TERMS else 65
    enc = SR.encodings(oracle, n, terms)[0]
    want = SR.want_wire(oracle, n, terms)[0]
    for where in ("device", "host"):
        e, out = place(enc, where), place(np.full((n, 32), 0xEE, dtype=np.uint8), where)
        eng._follow_torch_stream(e) if where == "device" else None
        assert eng.lib.zc_ris_sum_rows(eng.ctx, v(e), terms, v(out), None, n) == 0
        eng.synchronize()
        assert np.array_equal(host(out), want)


@pytest.mark.parametrize("terms", [1, 2, 8, 32])
def test_serial_rows_agree_with_zc_ed_fold_ordered(eng, oracle, terms):
    pts = SR.points(oracle, 65, terms)
    got = host(eng.ed_sum_rows(dev(pts)))
    for i in (0, 1, 2, 5, 7, 64):
        one = np.zeros(20, dtype=np.uint64)
        assert eng.lib.zc_ed_fold_ordered(eng.ctx, v(np.ascontiguousarray(pts[i])), terms, v(one)) == 0
        assert np.array_equal(one, got[i]), i
    if terms == 1:
        assert np.array_equal(got, pts[:, 0])


@pytest.mark.parametrize("terms", [3, 32, 33, 47])
def test_limbs_do_not_depend_on_placement_batch_size_or_neighbours(eng, oracle, terms):
    pts = SR.points(oracle, 1000, terms)
    d1000, h1000 = host(eng.ed_sum_rows(dev(pts))), eng.ed_sum_rows(np.ascontiguousarray(pts))
    assert np.array_equal(d1000, h1000)
    for n in (1, 65, 300):
        assert np.array_equal(host(eng.ed_sum_rows(dev(pts[:n]))), d1000[:n]) and np.array_equal(eng.ed_sum_rows(np.ascontiguousarray(pts[:n])), d1000[:n])
    assert np.array_equal(host(eng.ed_sum_rows(dev(pts[37:137]))), d1000[37:137])
    enc = SR.encodings(oracle, 1000, terms)[0]
    w1000 = host(eng.ris_sum_rows(dev(enc))[0])
    assert np.array_equal(host(eng.ris_sum_rows(dev(enc[37:137]))[0]), w1000[37:137])


@pytest.mark.parametrize("terms", [3, 33, 512])
def test_a_hostile_row_leaves_every_other_row_alone(eng, oracle, terms):
    """One hostile row per workgroup position (the rows a workgroup holds: 256 / parts) in turn; every other row keeps its limbs
    and bytes."""
    n = 300 if terms < 100 else 20
    pts, enc = np.array(SR.points(oracle, n, terms)), np.array(SR.encodings(oracle, n, terms)[0])
    clean, cw = host(eng.ed_sum_rows(dev(pts))), host(eng.ris_sum_rows(dev(enc))[0])
    pats = [np.array(w, dtype=np.uint64) for _, w in HR.point_patterns(pts[0, 0].tolist())]
    bad = SR.undecodable(oracle)
    for k, i in enumerate((0, 1, 63, 64, 255, 256, n - 1) if n == 300 else (0, 7, 8, n - 1)):
        p2, e2 = pts.copy(), enc.copy()
        p2[i, :: max(1, terms // 3)] = pats[k % len(pats)]
        e2[i, terms // 2] = bad[k % len(bad)]
        others = np.arange(n) != i
        assert np.array_equal(host(eng.ed_sum_rows(dev(p2)))[others], clean[others]), i
        assert np.array_equal(host(eng.ris_sum_rows(dev(e2))[0])[others], cw[others]), i


# ------------------------------------------------------------------ framed buffers, alignment
def _framed_call(e, backend, fn):
    import torch
    if backend == "torch":
        e._follow_torch_stream(torch.empty(1, dtype=torch.uint8, device="cuda"))

    def call(ip, op):
        fn(ip, op)
        torch.cuda.synchronize()
        e.synchronize()
    return call


@pytest.mark.parametrize("backend,terms,n", [("torch", 3, 300), ("numpy", 3, 300), ("torch", 33, 300), ("numpy", 33, 300), ("torch", 600, 20), ("numpy", 600, 20),
                                             ("torch", 8192, 1)])              # (a frame is 256 rows: the long row on the device only)
def test_framed_buffers(eng, oracle, backend, terms, n):
    """Frames and inputs as they were under zero and hostile fills, rows on a 16-byte boundary and 8 bytes off one; the outputs
    are the same under all of them and the model's."""
    from dusk_zerocaf_amd import _lib
    pts, enc = SR.points(oracle, n, terms).reshape(n, 20 * terms), SR.encodings(oracle, n, terms)[0].reshape(n, 32 * terms)
    want, (wb, wok) = SR.want_ed(oracle, n, terms), SR.want_wire(oracle, n, terms)

    def ed(ip, op):
        _lib.check(eng.lib.zc_ed_sum_rows(eng.ctx, C.c_void_p(ip[0]), terms, C.c_void_p(op[0]), n), ED, eng.lib)

    def ris(ip, op):
        _lib.check(eng.lib.zc_ris_sum_rows(eng.ctx, C.c_void_p(ip[0]), terms, C.c_void_p(op[0]), C.c_void_p(op[1]), n), RIS, eng.lib)
    for name, fn, ins, outs, check in (
            (ED, ed, [("points", pts, FB.hostile_frame_rows("pt*%d" % terms, oracle))], [("out", n, 20, np.uint64)], lambda o: np.array_equal(o[0], want)),
            (RIS, ris, [("in32", enc, FB.hostile_frame_rows("enc32*%d" % terms, oracle))], [("out32", n, 32, np.uint8), ("ok", n, 0, np.uint8)],
             lambda o: np.array_equal(o[0], wb) and np.array_equal(o[1], wok))):
        call = _framed_call(eng, backend, fn)
        got = {}
        for fill in (FB.ZERO, FB.HOSTILE):
            for shift in (0, 8):
                got[fill, shift] = FB.run_framed(call, ins, outs, backend=backend, fill=fill, in_shifts=[shift], out_shifts=[shift] + [0] * (len(outs) - 1))
        first = got[FB.ZERO, 0]
        assert check(first), name
        for key, res in got.items():
            FB.same_outputs([o[0] for o in outs], first, res, "%s, %s" % (name, key))


# ------------------------------------------------------------------ two streams, one workspace
def test_two_calls_in_flight_on_two_streams_with_the_two_kernel_form(eng, oracle):
    """Both calls keep their partials in the slot's workspace; the second goes out under another torch stream without a host
    synchronisation in between.  Each must return what it returns alone."""
    import torch
    terms, n = 8197, 3
    a = dev(SR.points(oracle, n, terms))
    b = dev(np.ascontiguousarray(SR.points(oracle, n, terms)[::-1]))
    want_a, want_b = SR.want_ed(oracle, n, terms), SR.want_ed(oracle, n, terms)[::-1]
    from tests import async_cases as AC
    fP, fK = dev(AC.points(oracle, AC.FILLER_ROWS, 7)), dev(AC.scalars(AC.FILLER_ROWS, 7))      # the filler of tests/test_gpu_async_scratch.py
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    pending = []
    for order in (0, 1):
        first, second = (a, b) if order == 0 else (b, a)
        done = torch.cuda.Event()
        eng.ed_scalar_mul(fP, fK)                                                        # about a millisecond in front of the first call
        r1 = eng.ed_sum_rows(first)
        done.record()
        with torch.cuda.stream(side):
            r2 = eng.ed_sum_rows(second)
        pending.append(not done.query())                                                 # the first call had not finished when the second went out
        torch.cuda.synchronize()
        ra, rb = (r1, r2) if order == 0 else (r2, r1)
        assert np.array_equal(host(ra), want_a) and np.array_equal(host(rb), want_b), order
    print("first call still pending when the second was issued: %s" % pending)


# ------------------------------------------------------------------ argument checks
def test_no_rows_no_terms_the_limit_and_mixed_memory(eng, oracle):
    import torch
    lib = eng.lib
    pts, enc = SR.points(oracle, 4, 3), SR.encodings(oracle, 4, 3)[0]
    dp, de = dev(pts), dev(enc)
    out, out32, dok = (torch.full((4, 20), 0x6E, dtype=torch.int64, device="cuda"), torch.full((4, 32), 0xEE, dtype=torch.uint8, device="cuda"),
                       torch.full((4,), 0xEE, dtype=torch.uint8, device="cuda"))
    hout, hout32, hok = np.zeros((4, 20), dtype=np.uint64), np.zeros((4, 32), dtype=np.uint8), np.zeros(4, dtype=np.uint8)
    eng._follow_torch_stream(dp)
    assert lib.zc_ed_sum_rows(eng.ctx, v(dp), 3, v(out), 0) == 0 and lib.zc_ris_sum_rows(eng.ctx, v(de), 3, v(out32), v(dok), 0) == 0
    assert lib.zc_ed_sum_rows(eng.ctx, v(pts), 3, v(hout), 0) == 0
    torch.cuda.synchronize()
    assert (host(out) == 0x6E).all() and (host(out32) == 0xEE).all() and (host(dok) == 0xEE).all() and not hout.any()
    assert eng.ed_sum_rows(np.zeros((0, 3, 20), dtype=np.uint64)).shape == (0, 20)
    # terms == 0: identity rows, zero bytes with ok = 1
    for where in ("host", "device"):
        z = eng.ed_sum_rows(place(np.zeros((70, 0, 20), dtype=np.uint64), where))
        assert np.array_equal(host(z), SR.PC.ident_rows(70))
        zb, zok = eng.ris_sum_rows(place(np.zeros((70, 0, 32), dtype=np.uint8), where))
        assert not host(zb).any() and (host(zok) == 1).all()
    assert lib.zc_ed_sum_rows(eng.ctx, v(dp), 3, v(hout), 4) == ZC_ERR_MIXED_MEM and lib.zc_ed_sum_rows(eng.ctx, v(pts), 3, v(out), 4) == ZC_ERR_MIXED_MEM
    assert lib.zc_ris_sum_rows(eng.ctx, v(de), 3, v(hout32), v(hok), 4) == ZC_ERR_MIXED_MEM and lib.zc_ris_sum_rows(eng.ctx, v(enc), 3, v(out32), None, 4) == ZC_ERR_MIXED_MEM
    assert lib.zc_ris_sum_rows(eng.ctx, v(enc), 3, v(hout32), v(dok), 4) == ZC_ERR_MIXED_MEM
    for terms in (3, 1 << 20, (1 << 31) - 1, 1 << 31, 1 << 40):
        edge = -(-(1 << 31) // terms)                                                    # the first n with n * terms >= 2^31
        assert lib.zc_ed_sum_rows(eng.ctx, v(pts), terms, v(hout), edge) == ZC_ERR_BAD_ARG and err(eng) == "%s: n * terms must stay below 2^31" % ED
        assert lib.zc_ris_sum_rows(eng.ctx, v(enc), terms, v(hout32), v(hok), edge) == ZC_ERR_BAD_ARG and err(eng) == "%s: n * terms must stay below 2^31" % RIS
        assert lib.zc_ed_sum_rows(eng.ctx, None, terms, v(hout), edge) == ZC_ERR_BAD_ARG and err(eng) == "null pointer: points"
        assert lib.zc_ris_sum_rows(eng.ctx, v(enc), terms, None, v(hok), edge) == ZC_ERR_BAD_ARG and err(eng) == "null pointer: out32"
    torch.cuda.synchronize()
    assert (host(out) == 0x6E).all() and not hout.any() and not hout32.any() and not hok.any()
