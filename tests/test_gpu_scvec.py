"""GPU tier: the scalar vector ops (zc_sc_sum_rows, zc_sc_dot_rows, zc_sc_powers) through the Engine and the C ABI against the
Python integers of tests/scvec_rows.py: every shape of its list -- the general lengths, both sides of every threshold of the plan,
the row of 16 * 2^16 + 5 terms -- from host arrays and from device tensors; the shared b against the tiled form; the dot product
against zc_sc_sum_rows of zc_sc_mul and against a zc_sc_muladd chain; a dot product with a power row against Horner; hostile rows
at the first, middle and last row of a workgroup; framed buffers 8 bytes off a 16-byte boundary; two calls of the two-kernel form
in flight on two streams; the argument checks; and one round of an inner-product argument that never leaves the device."""
import ctypes as C
import random

import numpy as np
import pytest

from oracle import pymodel as pm
from tests import framed_buffers as FB
from tests import scvec_rows as R

pytestmark = pytest.mark.gpu

L = R.L
SUM, DOT, POW = "zc_sc_sum_rows", "zc_sc_dot_rows", "zc_sc_powers"
ZC_ERR_BAD_ARG, ZC_ERR_MIXED_MEM = -1, -5


@pytest.fixture(scope="module")
def eng():
    import dusk_zerocaf_amd as z
    e = z.Engine()
    yield e
    e.close()


def dev(x):
    import torch
    return torch.from_numpy(np.array(x, dtype=np.uint64).view(np.int64)).cuda()


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


def run(eng, op, ins, terms, where):
    ins = [place(x, where) for x in ins]
    if op == "sum":
        return eng.sc_sum_rows(ins[0])
    if op == "powers":
        return eng.sc_powers(ins[0], terms)
    return eng.sc_dot_rows(ins[0], ins[1], shared_b=op == "dot_shared")


# ------------------------------------------------------------------ the shape list, both placements
@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("n,terms", R.row_shapes())
def test_sums_and_dot_products_are_the_python_integers(eng, n, terms, where):
    ran = 0
    for key in R.cases():
        op, fam, kn, kt = key
        if op == "powers" or (kn, kt) != (n, terms):
            continue
        c = R.case(*key)
        got = run(eng, op, c[:-1], terms, where)
        assert isinstance(got, np.ndarray) == (where == "host") and tuple(got.shape) == (n, 5)
        bad = np.flatnonzero((host(got) != c[-1]).any(axis=1))
        assert len(bad) == 0, (R.label(*key), bad[:8])
        ran += 1
    assert ran >= 4


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("n,terms", R.pow_shapes())
def test_power_rows_are_the_python_integers(eng, n, terms, where):
    x, want = R.case("powers", "bases", n, terms)
    got = run(eng, "powers", [x], terms, where)
    assert isinstance(got, np.ndarray) == (where == "host") and tuple(got.shape) == (n, terms, 5)
    bad = np.argwhere((host(got) != want).any(axis=2))
    assert len(bad) == 0, bad[:8]
    if terms:
        assert (host(got)[:, 0] == np.array(pm.limbs(1), dtype=np.uint64)).all()         # x^0 = 1, also for x = 0 mod L


# ------------------------------------------------------------------ against what a caller composes today
@pytest.mark.parametrize("n,terms", [(65, 8), (3, 65), (257, 33), (3, 1025), (1, 32769)])
def test_shared_b_is_the_tiled_form(eng, n, terms):
    a, b, want = R.case("dot_shared", "random", n, terms)
    da, db = dev(a), dev(b)
    tiled = dev(np.ascontiguousarray(np.broadcast_to(b, (n, terms, 5))))
    shared = host(eng.sc_dot_rows(da, db, shared_b=True))
    assert np.array_equal(shared, host(eng.sc_dot_rows(da, tiled)))
    assert np.array_equal(shared, eng.sc_dot_rows(np.ascontiguousarray(a), np.ascontiguousarray(b), shared_b=True))      # one upload per device
    assert np.array_equal(shared, want)


@pytest.mark.parametrize("n,terms", [(257, 7), (64, 65), (3, 1025)])
def test_dot_is_the_sum_of_the_products_and_a_muladd_chain(eng, n, terms):
    a, b, want = R.case("dot", "edges" if n * terms <= R.EDGE_RECORDS_MAX else "random", n, terms)
    da, db = dev(a), dev(b)
    dot = host(eng.sc_dot_rows(da, db))
    prod = eng.sc_mul(da.reshape(n * terms, 5), db.reshape(n * terms, 5)).reshape(n, terms, 5)
    assert np.array_equal(dot, host(eng.sc_sum_rows(prod))) and np.array_equal(dot, want)
    acc = dev(np.zeros((n, 5), dtype=np.uint64))
    for j in range(min(terms, 65)):
        acc = eng.sc_muladd(da[:, j].contiguous(), db[:, j].contiguous(), acc)
    m = min(terms, 65)
    assert np.array_equal(host(acc), host(eng.sc_dot_rows(da[:, :m].contiguous(), db[:, :m].contiguous())))


@pytest.mark.parametrize("n,terms", [(65, 8), (3, 300), (1, 20000)])
def test_polynomial_evaluation_is_horner(eng, n, terms):
    rng = random.Random(R.SEED + terms)
    c = R.fill(n, terms, "random", R.SEED + 40 + terms)
    x = R.bases(n, R.SEED + 41 + terms)
    got = host(eng.sc_dot_rows(dev(c), eng.sc_powers(dev(x), terms)))
    cv, xv = R.vals(c), R.vals(x)
    for i in sorted({0, n // 2, n - 1, rng.randrange(n)}):
        acc = 0
        for j in reversed(range(terms)):
            acc = (acc * int(xv[i]) + int(cv[i, j])) % L
        assert got[i].tolist() == pm.limbs(acc), i
    # one point for every polynomial: the power row as a shared b (a Shamir dealer evaluates at one share index at a time)
    row = eng.sc_powers(dev(x[:1]), terms)[0].contiguous()
    shared = host(eng.sc_dot_rows(dev(c), row, shared_b=True))
    assert shared[0].tolist() == got[0].tolist()


# ------------------------------------------------------------------ rows do not touch each other
@pytest.mark.parametrize("terms", [3, 33, 300])
def test_hostile_rows_change_no_other_row(eng, terms):
    """Worst-magnitude and zero-by-value records planted in the first, a middle and the last row of a workgroup (the rows a
    workgroup holds: 256 / parts) and in the batch's last row; every other row keeps its limbs."""
    from tests import hostile_rows as HR
    rpb = 256 // next(p for p in (1, 4, 16, 64, 256) if terms <= 4 * p)                # 3: 256 rows of a workgroup, 33: 16, 300: 1
    n = max(2 * rpb + 5, 40)
    a, b = R.fill(n, terms, "random", 90 + terms), R.fill(n, terms, "random", 91 + terms)
    x = R.fill(n, 1, "random", 92 + terms)[:, 0]
    clean = [host(eng.sc_sum_rows(dev(a))), host(eng.sc_dot_rows(dev(a), dev(b))), host(eng.sc_powers(dev(x), terms)).reshape(n, -1)]
    S = sorted({0, rpb // 2, rpb - 1, rpb, n - 1})
    pats = [("all ones", [R.ALL_ONES] * 5), ("L", pm.limbs(L)), ("high bits only", [R.HIGH, 0, 0, 0, R.ALL_ONES & ~R.M52]), ("2^260 - 1", pm.limbs(R.WORST))]
    for turn in range(2):
        a2, b2, x2 = a.copy(), b.copy(), x.copy()
        for k, i in enumerate(S):
            w = np.array(pats[(k + turn) % len(pats)][1], dtype=np.uint64)
            a2[i, :: max(1, terms // 3)] = w
            b2[i] = w
            x2[i] = w
        hostile = [host(eng.sc_sum_rows(dev(a2))), host(eng.sc_dot_rows(dev(a2), dev(b2))), host(eng.sc_powers(dev(x2), terms)).reshape(n, -1)]
        for what, c, h in zip((SUM, DOT, POW), clean, hostile):
            HR.assert_others_unchanged(c, h, S, what)
        assert np.array_equal(hostile[0], R.sum_expected(a2)) and np.array_equal(hostile[1], R.dot_expected(a2, b2))


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


@pytest.mark.parametrize("backend,terms,n", [("torch", 3, 300), ("numpy", 3, 300), ("torch", 65, 40), ("numpy", 65, 40), ("torch", 1025, 3), ("torch", 32769, 1)])
def test_framed_buffers(eng, backend, terms, n):
    """Frames and inputs as they were under zero and hostile fills, rows on a 16-byte boundary and 8 bytes off one; the outputs
    are the same under all of them and the Python integers."""
    from dusk_zerocaf_amd import _lib
    a, b = R.fill(n, terms, "random", 70 + terms), R.fill(n, terms, "random", 71 + terms)
    x = R.bases(n, 72 + terms)
    pt = min(terms, 1025)                                                             # the power rows: n * pt records of output
    want = {SUM: R.sum_expected(a), DOT: R.dot_expected(a, b), DOT + " shared": R.dot_expected(a, np.broadcast_to(b[:1], a.shape)),
            POW: R.powers_expected(x, pt).reshape(n * pt, 5)}
    flat = lambda r: r.reshape(-1, 5)                                                 # framed as records: a frame is 256 records, not 256 rows
    hostile = FB.hostile_frame_rows("sc")

    def s(ip, op):
        _lib.check(eng.lib.zc_sc_sum_rows(eng.ctx, C.c_void_p(ip[0]), terms, C.c_void_p(op[0]), n), SUM, eng.lib)

    def d(ip, op):
        _lib.check(eng.lib.zc_sc_dot_rows(eng.ctx, C.c_void_p(ip[0]), C.c_void_p(ip[1]), terms, 0, C.c_void_p(op[0]), n), DOT, eng.lib)

    def ds(ip, op):
        _lib.check(eng.lib.zc_sc_dot_rows(eng.ctx, C.c_void_p(ip[0]), C.c_void_p(ip[1]), terms, 1, C.c_void_p(op[0]), n), DOT, eng.lib)

    def p(ip, op):
        _lib.check(eng.lib.zc_sc_powers(eng.ctx, C.c_void_p(ip[0]), pt, C.c_void_p(op[0]), n), POW, eng.lib)
    for name, fn, ins, outs in (
            (SUM, s, [("a", flat(a), hostile)], [("out", n, 5, np.uint64)]),
            (DOT, d, [("a", flat(a), hostile), ("b", flat(b), hostile)], [("out", n, 5, np.uint64)]),
            (DOT + " shared", ds, [("a", flat(a), hostile), ("b", flat(b[:1]), hostile)], [("out", n, 5, np.uint64)]),
            (POW, p, [("x", x, hostile)], [("out", n * pt, 5, np.uint64)])):
        call = _framed_call(eng, backend, fn)
        got = {}
        for fill in (FB.ZERO, FB.HOSTILE):
            for shift in (0, 8):
                got[fill, shift] = FB.run_framed(call, ins, outs, backend=backend, fill=fill, in_shifts=[shift] * len(ins), out_shifts=[shift])
        first = got[FB.ZERO, 0]
        assert np.array_equal(first[0], want[name]), name
        for key, res in got.items():
            FB.same_outputs([o[0] for o in outs], first, res, "%s, %s" % (name, key))


# ------------------------------------------------------------------ two streams, one workspace
def test_two_calls_in_flight_on_two_streams_with_the_two_kernel_form(eng, oracle):
    """Both calls keep their partials in the slot's workspace; the second goes out under another torch stream without a host
    synchronisation in between.  Each must return what it returns alone."""
    import torch
    from tests import async_cases as AC
    terms, n = 32769, 3
    a, b, want_a = R.case("dot", "random", n, terms)
    a2, b2 = np.ascontiguousarray(a[::-1]), np.ascontiguousarray(b[::-1])
    want_b = want_a[::-1]
    sa, ws_a = R.case("sum", "random", n, terms)
    da, db, da2, db2, dsa = dev(a), dev(b), dev(a2), dev(b2), dev(sa)
    fP, fK = dev(AC.points(oracle, AC.FILLER_ROWS, 7)), dev(AC.scalars(AC.FILLER_ROWS, 7))      # the filler of tests/test_gpu_async_scratch.py
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    pending = []
    for order in (0, 1):
        first, second = ((da, db), (da2, db2)) if order == 0 else ((da2, db2), (da, db))
        done = torch.cuda.Event()
        eng.ed_scalar_mul(fP, fK)                                                        # about a millisecond in front of the first call
        r1 = eng.sc_dot_rows(*first)
        done.record()
        with torch.cuda.stream(side):
            r2 = eng.sc_dot_rows(*second)
            r3 = eng.sc_sum_rows(dsa)
        pending.append(not done.query())                                                 # the first call had not finished when the second went out
        torch.cuda.synchronize()
        ra, rb = (r1, r2) if order == 0 else (r2, r1)
        assert np.array_equal(host(ra), want_a) and np.array_equal(host(rb), want_b) and np.array_equal(host(r3), ws_a), order
    print("first call still pending when the second was issued: %s" % pending)


# ------------------------------------------------------------------ argument checks
def test_no_rows_no_terms_flags_the_limit_and_mixed_memory(eng):
    import torch
    lib = eng.lib
    a, b = R.fill(4, 3, "random", 1), R.fill(4, 3, "random", 2)
    da, db = dev(a), dev(b)
    out = torch.full((4, 5), 0x6E, dtype=torch.int64, device="cuda")
    pout = torch.full((12, 5), 0x6E, dtype=torch.int64, device="cuda")
    hout, hp = np.zeros((4, 5), dtype=np.uint64), np.zeros((12, 5), dtype=np.uint64)
    eng._follow_torch_stream(da)
    assert lib.zc_sc_sum_rows(eng.ctx, v(da), 3, v(out), 0) == 0 and lib.zc_sc_dot_rows(eng.ctx, v(da), v(db), 3, 0, v(out), 0) == 0
    assert lib.zc_sc_dot_rows(eng.ctx, v(da), v(db), 3, 1, v(out), 0) == 0 and lib.zc_sc_powers(eng.ctx, v(da), 3, v(pout), 0) == 0
    assert lib.zc_sc_powers(eng.ctx, v(da), 0, v(pout), 4) == 0 and lib.zc_sc_powers(eng.ctx, v(a), 0, v(hp), 4) == 0        # terms == 0: nothing written
    assert lib.zc_sc_sum_rows(eng.ctx, v(a), 3, v(hout), 0) == 0
    torch.cuda.synchronize()
    assert (host(out) == 0x6E).all() and (host(pout) == 0x6E).all() and not hout.any() and not hp.any()
    assert eng.sc_sum_rows(np.zeros((0, 3, 5), dtype=np.uint64)).shape == (0, 5) and eng.sc_powers(np.zeros((0, 5), dtype=np.uint64), 3).shape == (0, 3, 5)
    for where in ("host", "device"):                                                      # terms == 0: zero rows
        z = place(np.zeros((70, 0, 5), dtype=np.uint64), where)
        assert not host(eng.sc_sum_rows(z)).any() and not host(eng.sc_dot_rows(z, z)).any() and host(eng.sc_sum_rows(z)).shape == (70, 5)
        assert tuple(eng.sc_powers(place(a[:, 0], where), 0).shape) == (4, 0, 5)
    for flags in (2, 3, 4, 1 << 31):
        assert lib.zc_sc_dot_rows(eng.ctx, v(a), v(b), 3, flags, v(hout), 4) == ZC_ERR_BAD_ARG and err(eng) == "zc_sc_dot_rows: unknown flag bits"
    assert lib.zc_sc_sum_rows(eng.ctx, v(da), 3, v(hout), 4) == ZC_ERR_MIXED_MEM and lib.zc_sc_sum_rows(eng.ctx, v(a), 3, v(out), 4) == ZC_ERR_MIXED_MEM
    for flags in (0, 1):
        assert lib.zc_sc_dot_rows(eng.ctx, v(da), v(b), 3, flags, v(out), 4) == ZC_ERR_MIXED_MEM
        assert lib.zc_sc_dot_rows(eng.ctx, v(a), v(db), 3, flags, v(hout), 4) == ZC_ERR_MIXED_MEM
        assert lib.zc_sc_dot_rows(eng.ctx, v(da), v(db), 3, flags, v(hout), 4) == ZC_ERR_MIXED_MEM
    assert lib.zc_sc_powers(eng.ctx, v(da), 3, v(hp), 4) == ZC_ERR_MIXED_MEM and lib.zc_sc_powers(eng.ctx, v(a), 3, v(pout), 4) == ZC_ERR_MIXED_MEM
    for terms in (3, 1 << 20, (1 << 31) - 1, 1 << 31, 1 << 40):
        edge = -(-(1 << 31) // terms)                                                    # the first n with n * terms >= 2^31
        for name, call in ((SUM, lambda n: lib.zc_sc_sum_rows(eng.ctx, v(a), terms, v(hout), n)), (DOT, lambda n: lib.zc_sc_dot_rows(eng.ctx, v(a), v(b), terms, 1, v(hout), n)),
                           (POW, lambda n: lib.zc_sc_powers(eng.ctx, v(a), terms, v(hp), n))):
            assert call(edge) == ZC_ERR_BAD_ARG and err(eng) == "%s: n * terms must stay below 2^31" % name
        assert lib.zc_sc_dot_rows(eng.ctx, v(a), None, terms, 0, v(hout), edge) == ZC_ERR_BAD_ARG and err(eng) == "null pointer: b"
        assert lib.zc_sc_powers(eng.ctx, None, terms, v(hp), edge) == ZC_ERR_BAD_ARG and err(eng) == "null pointer: x"
    torch.cuda.synchronize()
    assert (host(out) == 0x6E).all() and not hout.any() and not hp.any()


# ------------------------------------------------------------------ an inner-product-argument round on the device
def test_an_inner_product_argument_round_never_leaves_the_device(eng, oracle):
    """a' = u a_L + u^-1 a_R, b' = u^-1 b_L + u b_R, G' = u^-1 G_L + u G_R with zc_sc_muladd and zc_ed_lincomb_shared on device
    tensors; then <a', b'> = <a, b> + u^2 <a_L, b_R> + u^-2 <a_R, b_L>, every inner product from zc_sc_dot_rows."""
    import torch
    m = 512
    rng = random.Random(R.SEED + 99)
    a, b = R.fill(1, m, "random", R.SEED + 60), R.fill(1, m, "random", R.SEED + 61)
    u = rng.randrange(1, L)
    ui = pow(u, -1, L)
    da, db = dev(a), dev(b)
    h = m // 2
    aL, aR, bL, bR = (t.contiguous() for t in (da[0, :h], da[0, h:], db[0, :h], db[0, h:]))
    U, UI = (dev(np.array([pm.limbs(s)] * h, dtype=np.uint64)) for s in (u, ui))
    a2 = eng.sc_muladd(U, aL, eng.sc_mul(UI, aR))
    b2 = eng.sc_muladd(UI, bL, eng.sc_mul(U, bR))
    k = dev(np.array([pm.limbs(rng.randrange(L)) for _ in range(m)], dtype=np.uint64))
    G = eng.ed_mul_base(k)                                                              # m generators
    G2 = eng.ed_lincomb_shared(torch.stack([G[:h], G[h:]], dim=1).contiguous(), [ui, u])
    dots = eng.sc_dot_rows(da, db)                                                      # <a, b>
    cross = eng.sc_dot_rows(torch.stack([aL, aR]).contiguous(), torch.stack([bR, bL]).contiguous())     # <a_L, b_R>, <a_R, b_L>
    folded = eng.sc_dot_rows(a2.reshape(1, h, 5), b2.reshape(1, h, 5))
    torch.cuda.synchronize()
    ab, (cl, cr) = int(R.vals(host(dots))[0]), [int(x) for x in R.vals(host(cross))]
    av, bv = R.vals(a)[0], R.vals(b)[0]
    assert ab == int((av * bv).sum() % L) and cl == int((av[:h] * bv[h:]).sum() % L) and cr == int((av[h:] * bv[:h]).sum() % L)
    assert host(folded)[0].tolist() == pm.limbs((ab + u * u * cl + ui * ui * cr) % L)
    # the folded generators are the ones a verifier would compute term by term
    scal = lambda s: dev(np.array([pm.limbs(s)] * h, dtype=np.uint64))
    want = eng.ed_add(eng.ed_scalar_mul(G[:h].contiguous(), scal(ui)), eng.ed_scalar_mul(G[h:].contiguous(), scal(u)))
    assert host(eng.ed_eq(G2, want)).all()
