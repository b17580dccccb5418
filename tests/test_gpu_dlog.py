"""GPU tier: the bounded discrete logs (zc_dlog_create, zc_dlog_destroy, zc_ed_dlog, zc_ris_dlog) through the C ABI against the
PLANTED truth of tests/dlog_rows.py: every found row is m * G from the oracle with m < bound, every other row is not found by
construction.  Tables of 2^4 and 2^9 records -- 2^4 with a bound past 1024 * 16 reaches the second launch by shape --, plain and
ZC_DLOG_COSET4, three generators (the basepoint, a multiple in other coordinates, a point of order 8 L), batches on both sides
of a wave with the m list cycled so that one wave holds rows that end in different chunks and launches, host arrays and device
tensors, encodings, hostile rows between good ones in framed buffers, ok = NULL, two live tables, ids of the other kinds, a
table made from a device-resident point, and the argument checks."""
import ctypes as C

import numpy as np
import pytest

from tests import dlog_rows as DR
from tests import framed_buffers as FB
from tests import gens_rows as GR

pytestmark = pytest.mark.gpu

BITS = (4, 9)
SIZES = [1, 63, 65, 300]
ZC_ERR_BAD_ARG, ZC_ERR_MIXED_MEM = -1, -5
UNKNOWN = "unknown dlog table"


@pytest.fixture(scope="module")
def eng():
    import dusk_zerocaf_amd as z
    e = z.Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def tables(eng, oracle):
    """(generator, bits, coset4) -> DlogTable, each created once from a host point."""
    out = {(g, t, c): eng.dlog_table(DR.generator(oracle, g), t, coset4=bool(c)) for g in DR.GENERATORS for t in BITS for c in (0, 1)}
    yield out
    for tb in out.values():
        tb.close()


def dev(x):
    import torch
    x = np.array(x, order="C")                                                          # a copy: the rows of tests/dlog_rows.py are read-only
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


def cycled(R, keys, n):
    i = np.arange(n) % len(R[keys[0]])
    return [np.ascontiguousarray(R[k][i]) for k in keys]


# ------------------------------------------------------------------ the planted truth
@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("coset4", [0, 1])
@pytest.mark.parametrize("t", BITS)
@pytest.mark.parametrize("name", DR.GENERATORS)
@pytest.mark.parametrize("n", SIZES)
def test_ed_rows_give_the_planted_m(eng, tables, oracle, n, name, t, coset4, where):
    R = DR.ed_rows(oracle, name, t, coset4)
    pts, want_m, want_found = cycled(R, ("points", "m", "found"), n)
    m, found, ok = tables[name, t, coset4].ed(place(pts, where), R["bound"])
    assert isinstance(m, np.ndarray) == (where == "host") and tuple(m.shape) == (n,) and tuple(found.shape) == (n,)
    bad = np.flatnonzero((host(found) != want_found) | (host(m) != want_m))
    assert len(bad) == 0, [(int(i), R["what"][i % len(R["what"])], int(host(m)[i]), int(host(found)[i])) for i in bad[:6]]
    assert host(ok).all()


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("t", BITS)
@pytest.mark.parametrize("name", DR.WIRE_GENERATORS)
@pytest.mark.parametrize("n", SIZES)
def test_encodings_give_the_planted_m_and_undecodable_rows_are_flagged(eng, tables, oracle, n, name, t, where):
    W = DR.wire_rows(oracle, name, t)
    k = len(W["enc"])
    order = (np.arange(n) * 7 + k - 7) % k                                              # the identity and undecodable rows from the first wave on
    m, found, ok = tables[name, t, 1].ris(place(W["enc"][order], where), W["bound"])
    assert np.array_equal(host(m), W["m"][order]) and np.array_equal(host(found), W["found"][order]) and np.array_equal(host(ok), W["ok"][order])


def test_the_answers_do_not_depend_on_batch_size_placement_or_a_larger_bound(eng, tables, oracle):
    for t in BITS:
        R = DR.ed_rows(oracle, "multiple", t, 0)
        pts, want_m, want_found = cycled(R, ("points", "m", "found"), 300)
        tb = tables["multiple", t, 0]
        m, found, _ = tb.ed(pts, R["bound"])
        for lo, hi in ((0, 1), (37, 137), (64, 129)):
            for where in ("device", "host"):
                m2, f2, _ = tb.ed(place(pts[lo:hi], where), R["bound"])
                assert np.array_equal(host(m2), m[lo:hi]) and np.array_equal(host(f2), found[lo:hi])
        big = 3 * R["bound"] + 11                                                       # rows found under both bounds: the same m
        m3, f3, _ = tb.ed(dev(pts), big)
        hit = found == 1
        assert np.array_equal(host(m3)[hit], m[hit]) and host(f3)[hit].all()
        between = [i for i, w in enumerate(R["what"]) if w.startswith("m=%d (" % R["bound"])]
        assert between and all(host(f3)[i] == 1 and host(m3)[i] == R["bound"] for i in between)     # the row at the old bound is found under the larger one


def test_e4_is_absorbed_by_coset4_tables_only(eng, tables, oracle):
    R0, R1 = DR.ed_rows(oracle, "B", 9, 0), DR.ed_rows(oracle, "B", 9, 1)
    assert np.array_equal(R0["points"], R1["points"])
    t4 = [i for i, w in enumerate(R0["what"]) if " + 2 T8" in w or " + 4 T8" in w or " + 6 T8" in w]
    t8 = [i for i, w in enumerate(R0["what"]) if " + 1 T8" in w or " + 3 T8" in w or " + 5 T8" in w or " + 7 T8" in w]
    assert len(t4) == 18 and len(t8) == 24
    assert not R0["found"][t4].any() and R1["found"][t4].all() and not R0["found"][t8].any() and not R1["found"][t8].any()
    for c, R in ((0, R0), (1, R1)):
        m, found, _ = tables["B", 9, c].ed(R["points"], R["bound"])
        assert np.array_equal(found, R["found"]) and np.array_equal(m, R["m"])


# ------------------------------------------------------------------ hostile rows, framed buffers, ok = NULL
def raw(e, name, tid, rows, bound, m, found, ok, n):
    from dusk_zerocaf_amd import _lib
    _lib.check(getattr(e.lib, name)(e.ctx, C.c_uint64(tid), C.c_void_p(rows), C.c_uint64(bound), C.c_void_p(m), C.c_void_p(found), C.c_void_p(ok) if ok else None, n), name, e.lib)


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
@pytest.mark.parametrize("t", BITS)
def test_hostile_rows_between_good_rows_in_framed_buffers(eng, tables, oracle, backend, t):
    """Every fourth row is off the curve, has Z = 0 by value or all-ones limbs: ok = 0, found = 0, m = 0 there, the good rows'
    answers as without them, nothing outside rows 0 .. n-1 written, the same outputs under zero and hostile frames and 8 bytes
    off a 16-byte boundary."""
    n = 300
    R = DR.ed_rows(oracle, "mixed", t, 0)
    pts, want_m, want_found = cycled(R, ("points", "m", "found"), n)
    pts, want_m, want_found, want_ok = pts.copy(), want_m.copy(), want_found.copy(), np.ones(n, dtype=np.uint8)
    hostile = DR.hostile_points(oracle)
    for i in range(1, n, 4):
        pts[i] = hostile[(i // 4) % 3]
        want_m[i], want_found[i], want_ok[i] = 0, 0, 0
    tid = tables["mixed", t, 0].id
    outs = [("m_out", n, 0, np.uint64), ("found", n, 0, np.uint8), ("ok", n, 0, np.uint8)]
    call = _framed_call(eng, backend, lambda ip, op: raw(eng, "zc_ed_dlog", tid, ip[0], R["bound"], op[0], op[1], op[2], n))
    got = {}
    for fill in (FB.ZERO, FB.HOSTILE):
        for shift in (0, 8):
            got[fill, shift] = FB.run_framed(call, [("p", pts, FB.hostile_frame_rows("pt", oracle))], outs, backend=backend, fill=fill, in_shifts=[shift], out_shifts=[shift] * 3)
    first = got[FB.ZERO, 0]
    assert np.array_equal(first[0], want_m) and np.array_equal(first[1], want_found) and np.array_equal(first[2], want_ok)
    for key, res in got.items():
        FB.same_outputs([o[0] for o in outs], first, res, "zc_ed_dlog, %s" % (key,))


@pytest.mark.parametrize("backend", ["torch", "numpy"])
def test_encodings_in_framed_buffers_and_ok_null(eng, tables, oracle, backend):
    n = 130
    W = DR.wire_rows(oracle, "B", 4)
    order = (np.arange(n) * 5 + len(W["enc"]) - 9) % len(W["enc"])
    enc = np.ascontiguousarray(W["enc"][order])
    tid = tables["B", 4, 1].id
    outs = [("m_out", n, 0, np.uint64), ("found", n, 0, np.uint8), ("ok", n, 0, np.uint8)]
    call = _framed_call(eng, backend, lambda ip, op: raw(eng, "zc_ris_dlog", tid, ip[0], W["bound"], op[0], op[1], op[2], n))
    res = FB.run_framed(call, [("in32", enc, FB.hostile_frame_rows("enc32", oracle))], outs, backend=backend, fill=FB.HOSTILE, in_shifts=[8], out_shifts=[8, 8, 8])
    assert np.array_equal(res[0], W["m"][order]) and np.array_equal(res[1], W["found"][order]) and np.array_equal(res[2], W["ok"][order])
    # ok = NULL: the same m and found, and the third buffer is not touched
    null = _framed_call(eng, backend, lambda ip, op: raw(eng, "zc_ris_dlog", tid, ip[0], W["bound"], op[0], op[1], None, n))
    res2 = FB.run_framed(null, [("in32", enc, FB.hostile_frame_rows("enc32", oracle))], outs, backend=backend, fill=FB.ZERO)
    assert np.array_equal(res2[0], res[0]) and np.array_equal(res2[1], res[1]) and (res2[2] == FB.OUT_ROW_FILL).all()
    R = DR.ed_rows(oracle, "B", 4, 0)
    pts = np.ascontiguousarray(R["points"][:70])
    edn = _framed_call(eng, backend, lambda ip, op: raw(eng, "zc_ed_dlog", tables["B", 4, 0].id, ip[0], R["bound"], op[0], op[1], None, 70))
    res3 = FB.run_framed(edn, [("p", pts, FB.hostile_frame_rows("pt", oracle))], [("m_out", 70, 0, np.uint64), ("found", 70, 0, np.uint8), ("ok", 70, 0, np.uint8)], backend=backend)
    assert np.array_equal(res3[0], R["m"][:70]) and np.array_equal(res3[1], R["found"][:70]) and (res3[2] == FB.OUT_ROW_FILL).all()


# ------------------------------------------------------------------ tables
def test_two_live_tables_used_alternately_then_one_destroyed(eng, oracle):
    Ra, Rb = DR.ed_rows(oracle, "B", 4, 0), DR.ed_rows(oracle, "multiple", 9, 1)
    a, b = eng.dlog_table(DR.generator(oracle, "B"), 4), eng.dlog_table(DR.generator(oracle, "multiple"), 9, coset4=True)
    assert a.id and b.id and a.id != b.id
    for _ in range(2):
        ma, fa, _ = a.ed(dev(Ra["points"]), Ra["bound"])
        mb, fb, _ = b.ed(Rb["points"], Rb["bound"])
        assert np.array_equal(host(ma), Ra["m"]) and np.array_equal(host(fa), Ra["found"]) and np.array_equal(mb, Rb["m"]) and np.array_equal(fb, Rb["found"])
    old = a.id
    a.close()
    m, f = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint8)
    p4 = np.ascontiguousarray(Ra["points"][1:5])
    assert eng.lib.zc_ed_dlog(eng.ctx, old, v(p4), 64, v(m), v(f), None, 4) == ZC_ERR_BAD_ARG and err(eng) == UNKNOWN and not m.any() and not f.any()
    assert eng.lib.zc_dlog_destroy(eng.ctx, old) == ZC_ERR_BAD_ARG and err(eng) == UNKNOWN
    mb, fb, _ = b.ed(dev(Rb["points"]), Rb["bound"])
    assert np.array_equal(host(mb), Rb["m"]) and np.array_equal(host(fb), Rb["found"])
    c = eng.dlog_table(DR.generator(oracle, "B"), 4)
    assert c.id not in (old, b.id)                                                       # ids are never reused
    assert np.array_equal(c.ed(Ra["points"], Ra["bound"])[0], Ra["m"])
    b.close()
    c.close()


def test_a_table_created_from_a_device_resident_point(eng, tables, oracle):
    R = DR.ed_rows(oracle, "multiple", 9, 1)
    with eng.dlog_table(dev(DR.generator(oracle, "multiple").reshape(1, 20)), 9, coset4=True) as tb:
        m, found, ok = tb.ed(dev(R["points"]), R["bound"])
        assert np.array_equal(host(m), R["m"]) and np.array_equal(host(found), R["found"]) and host(ok).all()
        W = DR.wire_rows(oracle, "multiple", 9)
        m, found, ok = tb.ris(W["enc"], W["bound"])
        assert np.array_equal(m, W["m"]) and np.array_equal(found, W["found"]) and np.array_equal(ok, W["ok"])


def test_ids_of_the_other_kinds_are_refused(eng, tables, oracle):
    lib = eng.lib
    R = DR.ed_rows(oracle, "B", 4, 0)
    p4, m, f = np.ascontiguousarray(R["points"][1:5]), np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint8)
    e4 = np.zeros((4, 32), dtype=np.uint8)
    pts = GR.with_true_t(oracle, GR.generators(oracle, 2))
    tid = tables["B", 4, 0].id
    with eng.msm_bases(pts) as mb, eng.generators(pts) as gs:
        for other in (mb.id, gs.id, 0, tid + (1 << 40)):
            assert lib.zc_ed_dlog(eng.ctx, other, v(p4), 64, v(m), v(f), None, 4) == ZC_ERR_BAD_ARG and err(eng) == UNKNOWN
            assert lib.zc_ris_dlog(eng.ctx, other, v(e4), 64, v(m), v(f), None, 4) == ZC_ERR_BAD_ARG and err(eng) == UNKNOWN
            assert lib.zc_dlog_destroy(eng.ctx, other) == ZC_ERR_BAD_ARG and err(eng) == UNKNOWN
        K = GR.scalars(2, 4)
        out = np.zeros((4, 20), dtype=np.uint64)
        assert lib.zc_ed_mul_gens(eng.ctx, tid, v(K), v(out), 4) == ZC_ERR_BAD_ARG and err(eng) == "unknown generator set"
        assert lib.zc_gens_destroy(eng.ctx, tid) == ZC_ERR_BAD_ARG and lib.zc_msm_bases_destroy(eng.ctx, tid) == ZC_ERR_BAD_ARG
        assert eng.ed_mul_gens(gs, K).shape == (4, 20) and mb.msm(np.ascontiguousarray(K[0])).shape == (1, 20)     # they are still there
    assert not m.any() and not f.any()
    got = tables["B", 4, 0].ed(p4, 64)
    assert np.array_equal(got[0], R["m"][1:5]) and got[1].all()                                                    # and so is the table


def test_a_table_of_another_context_is_foreign_and_goes_with_its_context(tables, oracle):
    import dusk_zerocaf_amd as z
    other = z.Engine()
    try:
        R = DR.ed_rows(oracle, "B", 4, 0)
        p4, m, f = np.ascontiguousarray(R["points"][1:5]), np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint8)
        assert other.lib.zc_ed_dlog(other.ctx, tables["B", 4, 0].id, v(p4), 64, v(m), v(f), None, 4) == ZC_ERR_BAD_ARG and err(other) == UNKNOWN
        tb = other.dlog_table(DR.generator(oracle, "B"), 4)                              # left live: zc_ctx_destroy frees it
        assert np.array_equal(tb.ed(p4, 64)[0], R["m"][1:5])
        tb.id = 0
    finally:
        other.close()


def test_create_refuses_bad_generators_and_leaves_nothing_behind(eng, oracle):
    import torch
    lib = eng.lib
    hostile = DR.hostile_points(oracle)
    tors = DR.PC.torsion(oracle)
    for where in ("host", "device"):
        for flags in (0, 1):
            for p in hostile[:2]:
                tid = C.c_uint64(0xFEED)
                held = place(p.reshape(1, 20), where)
                assert lib.zc_dlog_create(eng.ctx, v(held), 4, flags, C.byref(tid)) == ZC_ERR_BAD_ARG
                assert err(eng) == "zc_dlog_create: not a point of the curve" and tid.value == 0xFEED
            for j in range(8):
                tid = C.c_uint64(0xFEED)
                held = place(tors[j].reshape(1, 20), where)
                assert lib.zc_dlog_create(eng.ctx, v(held), 4, flags, C.byref(tid)) == ZC_ERR_BAD_ARG
                assert err(eng) == "zc_dlog_create: generator lies in E[8]" and tid.value == 0xFEED
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    tid = C.c_uint64(0)
    for _ in range(50):
        assert lib.zc_dlog_create(eng.ctx, v(np.ascontiguousarray(tors[1])), 22, 0, C.byref(tid)) == ZC_ERR_BAD_ARG
    assert free0 - torch.cuda.mem_get_info()[0] < 256 << 20 and tid.value == 0
    B = GR.basepoint()
    for bits in (0, 3, 23, 64):
        assert lib.zc_dlog_create(eng.ctx, v(B), bits, 0, C.byref(tid)) == ZC_ERR_BAD_ARG and err(eng) == "zc_dlog_create: table_bits must be ZC_DLOG_MIN_BITS .. ZC_DLOG_MAX_BITS"
    for flags in (2, 3, 1 << 31):
        assert lib.zc_dlog_create(eng.ctx, v(B), 4, flags, C.byref(tid)) == ZC_ERR_BAD_ARG and err(eng) == "zc_dlog_create: unknown flag bits"
    assert tid.value == 0


# ------------------------------------------------------------------ argument checks
def test_no_rows_mixed_memory_the_bound_and_the_order_of_the_checks(eng, tables, oracle):
    import torch
    lib = eng.lib
    plain, coset = tables["B", 4, 0].id, tables["B", 4, 1].id
    R = DR.ed_rows(oracle, "B", 4, 0)
    p4, e4 = np.ascontiguousarray(R["points"][1:5]), np.ascontiguousarray(DR.wire_rows(oracle, "B", 4)["enc"][1:5])
    dp, de = dev(p4), dev(e4)
    dm, df = torch.full((4,), 0x6E, dtype=torch.int64, device="cuda"), torch.full((4,), 0xEE, dtype=torch.uint8, device="cuda")
    hm, hf = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint8)
    eng._follow_torch_stream(dp)
    assert lib.zc_ed_dlog(eng.ctx, plain, v(dp), 64, v(dm), v(df), None, 0) == 0 and lib.zc_ris_dlog(eng.ctx, coset, v(de), 64, v(dm), v(df), None, 0) == 0
    assert lib.zc_ed_dlog(eng.ctx, plain, v(p4), 64, v(hm), v(hf), None, 0) == 0
    torch.cuda.synchronize()
    assert (host(dm) == 0x6E).all() and (host(df) == 0xEE).all() and not hm.any() and not hf.any()
    assert lib.zc_ed_dlog(eng.ctx, plain, v(dp), 64, v(hm), v(df), None, 4) == ZC_ERR_MIXED_MEM
    assert lib.zc_ed_dlog(eng.ctx, plain, v(p4), 64, v(hm), v(hf), v(df), 4) == ZC_ERR_MIXED_MEM
    assert lib.zc_ris_dlog(eng.ctx, coset, v(e4), 64, v(dm), v(hf), None, 4) == ZC_ERR_MIXED_MEM
    assert lib.zc_ris_dlog(eng.ctx, plain, v(e4), 64, v(hm), v(hf), None, 4) == ZC_ERR_BAD_ARG and err(eng) == "zc_ris_dlog needs a ZC_DLOG_COSET4 table"
    for name, tid, rows, rname in (("zc_ed_dlog", plain, p4, "p"), ("zc_ris_dlog", coset, e4, "in32")):
        fn = getattr(lib, name)
        assert fn(eng.ctx, 0, None, 0, v(hm), v(hf), None, 0) == ZC_ERR_BAD_ARG and err(eng) == "null pointer: %s" % rname     # the pointers before the id, the bound and n == 0
        assert fn(eng.ctx, 0, v(rows), 0, None, v(hf), None, 0) == ZC_ERR_BAD_ARG and err(eng) == "null pointer: m_out"
        assert fn(eng.ctx, 0, v(rows), 0, v(hm), None, None, 0) == ZC_ERR_BAD_ARG and err(eng) == "null pointer: found"
        assert fn(eng.ctx, 0, v(rows), 0, v(hm), v(hf), None, 0) == ZC_ERR_BAD_ARG and err(eng) == UNKNOWN                      # the id before the bound
        for bound in (0, (65536 << 4) + 1, 1 << 63):
            assert fn(eng.ctx, tid, v(rows), bound, v(hm), v(hf), None, 0) == ZC_ERR_BAD_ARG and err(eng) == "%s: bound must be 1 .. 2^table_bits * ZC_DLOG_MAX_STEPS" % name
        assert fn(eng.ctx, tid, v(rows), 64, v(hm), v(hf), None, 1 << 31) == ZC_ERR_BAD_ARG and err(eng) == "%s: n must stay below 2^31" % name
    assert tables["B", 4, 0].ed(np.zeros((0, 20), dtype=np.uint64), 5)[0].shape == (0,)
    torch.cuda.synchronize()
    assert (host(dm) == 0x6E).all() and not hm.any() and not hf.any()


def test_the_largest_bound_of_a_small_table_runs_all_64_launches(eng, tables, oracle):
    """t = 4, bound = 2^4 * 65536: m = bound - 1 sits in the last giant step of the last launch."""
    bound = 65536 << 4
    G = DR.generator(oracle, "B")
    pts = DR.multiples(oracle, G, [bound - 1, bound, 63 * 1024 * 16, 5])
    m, found, ok = tables["B", 4, 0].ed(dev(pts), bound)
    assert host(m).tolist() == [bound - 1, 0, 63 * 1024 * 16, 5] and host(found).tolist() == [1, 0, 1, 1] and host(ok).all()
