"""GPU tier: the generator sets (zc_gens_create, zc_gens_destroy, zc_ed_mul_gens, zc_ris_mul_gens_compress) through the C ABI
against the oracle (zc_ref).  Generator lists of 1, 2, 3 and 8 points from every class of tests/point_classes.py, host arrays and
device tensors, batch sizes on both sides of a wave and of a workgroup, framed buffers, two live sets, a set made from
device-resident points, the refusals of zc_gens_create, ids of the other kind, and the argument checks.  The rows are those of
tests/gens_rows.py (96 distinct rows per count, every edge scalar in every term position, repeated for longer batches); the
oracle's answers are computed once per count.  Every scalar pattern is legal input."""
import ctypes as C

import numpy as np
import pytest

from tests import framed_buffers as FB
from tests import gens_rows as GR

pytestmark = pytest.mark.gpu

CREATE, DESTROY, ED, RIS = "zc_gens_create", "zc_gens_destroy", "zc_ed_mul_gens", "zc_ris_mul_gens_compress"
SIZES = [1, 63, 65, 255, 257, 300, 1000]
ZC_ERR_BAD_ARG, ZC_ERR_MIXED_MEM = -1, -5
UNKNOWN = "unknown generator set"


@pytest.fixture(scope="module")
def eng():
    import dusk_zerocaf_amd as z
    e = z.Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def sets(eng, oracle):
    """count -> Generators, each created once from host points."""
    out = {count: eng.generators(GR.generators(oracle, count)) for count in GR.COUNTS}
    yield out
    for g in out.values():
        g.close()


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


# ------------------------------------------------------------------ counts, sizes, placements
@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("count", GR.COUNTS)
@pytest.mark.parametrize("n", SIZES)
def test_both_forms_are_the_oracles_sum(eng, sets, oracle, n, count, where):
    """zc_ed_eq = 1 against the oracle's ((k_0 G_0 + k_1 G_1) + ...), its compressed Edwards bytes, and the wire form's bytes
    equal to the oracle's ris_compress and to zc_ris_compress of the Edwards form's output."""
    K = GR.scalars(count, n)
    pts, enc = GR.want(oracle, count, n)
    got = eng.ed_mul_gens(sets[count], place(K, where))
    assert isinstance(got, np.ndarray) == (where == "host") and tuple(got.shape) == (n, 20)
    eq = host(eng.ed_eq(got, place(pts, where)))
    assert eq.all(), np.flatnonzero(eq == 0)[:8]
    gb, gok = eng.ed_compress(got)
    wb, wok = oracle.mt(oracle.ed_compress, np.ascontiguousarray(pts))
    assert np.array_equal(host(gb), wb) and np.array_equal(host(gok), wok)
    assert (host(got) <= GR.M52).all()
    wire = eng.ris_mul_gens_compress(sets[count], place(K, where))
    assert isinstance(wire, np.ndarray) == (where == "host") and tuple(wire.shape) == (n, 32)
    assert np.array_equal(host(wire), enc), np.flatnonzero((host(wire) != enc).any(axis=1))[:8]
    assert np.array_equal(host(wire), host(eng.ris_compress(got)))


@pytest.mark.parametrize("count", GR.COUNTS)
def test_limbs_do_not_depend_on_placement_or_batch_size(eng, sets, count):
    K = GR.scalars(count, 1000)
    d1000, h1000 = host(eng.ed_mul_gens(sets[count], dev(K))), eng.ed_mul_gens(sets[count], K)
    assert np.array_equal(d1000, h1000)
    for n in (1, 65, 300):
        assert np.array_equal(host(eng.ed_mul_gens(sets[count], dev(K[:n]))), d1000[:n]) and np.array_equal(eng.ed_mul_gens(sets[count], K[:n]), d1000[:n])
    shifted = host(eng.ed_mul_gens(sets[count], dev(K[37:137])))                         # other rows share the wave: the same limbs
    assert np.array_equal(shifted, d1000[37:137])


def test_identity_sums_give_32_zero_bytes(eng, sets, oracle):
    pool, _ = GR.scalar_pool()
    same = np.ascontiguousarray(np.stack([pool, pool], axis=1))                          # k G - k G
    assert GR.PC.is_identity(oracle, eng.ed_mul_gens(sets[2], same)).all() and not eng.ris_mul_gens_compress(sets[2], same).any()
    zero = np.zeros((130, 8, 5), dtype=np.uint64)
    assert GR.PC.is_identity(oracle, host(eng.ed_mul_gens(sets[8], dev(zero)))).all() and not host(eng.ris_mul_gens_compress(sets[8], dev(zero))).any()


def test_the_list_of_the_basepoint_agrees_with_the_basepoint_calls(eng, oracle):
    K = GR.scalars(1, 1000)
    k = np.ascontiguousarray(K[:, 0])
    with eng.generators(GR.basepoint()) as g:
        for where in ("device", "host"):
            got = eng.ed_mul_gens(g, place(K, where))
            assert host(eng.ed_eq(got, eng.ed_mul_base(place(k, where)))).all()
            assert np.array_equal(host(eng.ris_mul_gens_compress(g, place(K, where))), host(eng.ris_mul_base_compress(place(k, where))))
        assert np.array_equal(eng.ris_mul_gens_compress(g, K), GR.want_base(oracle, 1000)[1])


# ------------------------------------------------------------------ framed buffers
def raw(e, name, gid, *args):
    from dusk_zerocaf_amd import _lib
    _lib.check(getattr(e.lib, name)(e.ctx, C.c_uint64(gid), *[C.c_void_p(a) for a in args[:-1]], args[-1]), name, e.lib)


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
@pytest.mark.parametrize("count", [1, 3, 8])
def test_framed_buffers(eng, sets, oracle, backend, count):
    """n = 300: frames and inputs as they were under zero and hostile fills, rows on a 16-byte boundary and 8 bytes off one; the
    outputs are the same under all of them and the oracle's."""
    n = 300
    K = GR.scalars(count, n).reshape(n, 5 * count)
    pts, enc = GR.want(oracle, count, n)
    frames = FB.hostile_frame_rows("sc*%d" % count if count > 1 else "sc", oracle)
    gid = sets[count].id
    for name, out, check in ((ED, ("out", n, 20, np.uint64), lambda o: oracle.ed_eq(o, np.ascontiguousarray(pts)).all()),
                             (RIS, ("out32", n, 32, np.uint8), lambda o: np.array_equal(o, enc))):
        call = _framed_call(eng, backend, lambda ip, op, name=name: raw(eng, name, gid, ip[0], op[0], n))
        got = {}
        for fill in (FB.ZERO, FB.HOSTILE):
            for shift in (0, 8):
                got[fill, shift] = FB.run_framed(call, [("scalars", K, frames)], [out], backend=backend, fill=fill, in_shifts=[shift], out_shifts=[shift])
        first = got[FB.ZERO, 0]
        assert check(first[0]), name
        for key, res in got.items():
            FB.same_outputs([out[0]], first, res, "%s, %s" % (name, key))


# ------------------------------------------------------------------ sets
def test_two_live_sets_used_alternately_then_one_destroyed(eng, oracle):
    n = 300
    K2, K3 = GR.scalars(2, n), GR.scalars(3, n)
    w2, w3 = GR.want(oracle, 2, n)[1], GR.want(oracle, 3, n)[1]
    a, b = eng.generators(GR.generators(oracle, 2)), eng.generators(GR.generators(oracle, 3))
    assert a.id and b.id and a.id != b.id
    for _ in range(2):
        assert np.array_equal(host(eng.ris_mul_gens_compress(a, dev(K2))), w2) and np.array_equal(eng.ris_mul_gens_compress(b, K3), w3)
        assert np.array_equal(eng.ris_mul_gens_compress(a, K2), w2) and np.array_equal(host(eng.ris_mul_gens_compress(b, dev(K3))), w3)
    old = a.id
    a.close()
    out = np.zeros((n, 32), dtype=np.uint8)
    assert eng.lib.zc_ris_mul_gens_compress(eng.ctx, old, v(K2), v(out), n) == ZC_ERR_BAD_ARG and err(eng) == UNKNOWN and not out.any()
    assert eng.lib.zc_ed_mul_gens(eng.ctx, old, v(K2), v(np.zeros((n, 20), dtype=np.uint64)), n) == ZC_ERR_BAD_ARG and err(eng) == UNKNOWN
    assert eng.lib.zc_gens_destroy(eng.ctx, old) == ZC_ERR_BAD_ARG and err(eng) == UNKNOWN
    assert np.array_equal(host(eng.ris_mul_gens_compress(b, dev(K3))), w3) and np.array_equal(eng.ris_mul_gens_compress(b, K3), w3)
    c = eng.generators(GR.generators(oracle, 2))
    assert c.id not in (old, b.id)                                                       # ids are never reused
    assert np.array_equal(eng.ris_mul_gens_compress(c, K2), w2)
    b.close()
    c.close()


@pytest.mark.parametrize("count", [1, 8])
def test_a_set_created_from_device_resident_points(eng, sets, oracle, count):
    K = GR.scalars(count, 257)
    with eng.generators(dev(GR.generators(oracle, count))) as g:
        assert np.array_equal(host(eng.ed_mul_gens(g, dev(K))), host(eng.ed_mul_gens(sets[count], dev(K))))     # the same tables: the same limbs
        assert np.array_equal(eng.ris_mul_gens_compress(g, K), GR.want(oracle, count, 257)[1])


def test_create_refuses_what_is_no_curve_point_and_leaves_nothing_behind(eng, oracle):
    """The index named is the first bad generator's; *id_out is not written; refused lists of eight leave no tables allocated
    (200 refusals would hold 865 MB)."""
    import torch
    lib = eng.lib
    for where in ("host", "device"):
        for name, pts, first in GR.refused_lists(oracle):
            gid = C.c_uint64(0xFEED)
            p = place(pts, where)
            assert lib.zc_gens_create(eng.ctx, v(p), len(pts), C.byref(gid)) == ZC_ERR_BAD_ARG, name
            assert err(eng) == "zc_gens_create: generator %d is not a point of the curve" % first and gid.value == 0xFEED, name
    bad8 = np.ascontiguousarray(np.tile(GR.refused_lists(oracle)[1][1], (8, 1)))
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    gid = C.c_uint64(0)
    for _ in range(200):
        assert lib.zc_gens_create(eng.ctx, v(bad8), 8, C.byref(gid)) == ZC_ERR_BAD_ARG
    assert free0 - torch.cuda.mem_get_info()[0] < 256 << 20 and gid.value == 0
    for count in (0, 9):
        assert lib.zc_gens_create(eng.ctx, v(bad8), count, C.byref(gid)) == ZC_ERR_BAD_ARG and err(eng) == "zc_gens_create: count must be 1 .. ZC_GENS_MAX"


def test_ids_of_the_other_kind_are_refused(eng, sets, oracle):
    lib = eng.lib
    pts = GR.with_true_t(oracle, GR.generators(oracle, 2))
    K, out, out32 = GR.scalars(2, 4), np.zeros((4, 20), dtype=np.uint64), np.zeros((4, 32), dtype=np.uint8)
    with eng.msm_bases(pts) as mb:
        assert lib.zc_ed_mul_gens(eng.ctx, mb.id, v(K), v(out), 4) == ZC_ERR_BAD_ARG and err(eng) == UNKNOWN
        assert lib.zc_ris_mul_gens_compress(eng.ctx, mb.id, v(K), v(out32), 4) == ZC_ERR_BAD_ARG and err(eng) == UNKNOWN
        assert lib.zc_gens_destroy(eng.ctx, mb.id) == ZC_ERR_BAD_ARG and err(eng) == UNKNOWN
        assert mb.msm(np.ascontiguousarray(K[0])).shape == (1, 20)                       # the table is still there
    gid = sets[2].id
    sums = np.zeros((1, 20), dtype=np.uint64)
    assert lib.zc_msm_fixed(eng.ctx, gid, v(np.ascontiguousarray(K[0])), 1, v(sums)) == ZC_ERR_BAD_ARG and "no live table" in err(eng)
    assert lib.zc_msm_bases_destroy(eng.ctx, gid) == ZC_ERR_BAD_ARG and "no live table" in err(eng)
    assert np.array_equal(eng.ris_mul_gens_compress(sets[2], K), GR.want(oracle, 2, 4)[1])       # and so is the set
    for bad in (0, gid + (1 << 40)):
        assert lib.zc_ed_mul_gens(eng.ctx, bad, v(K), v(out), 4) == ZC_ERR_BAD_ARG and err(eng) == UNKNOWN
    assert not out.any() and not out32.any() and not sums.any()


def test_a_set_of_another_context_is_foreign(sets, oracle):
    import dusk_zerocaf_amd as z
    other = z.Engine()
    try:
        K, out = GR.scalars(2, 4), np.zeros((4, 20), dtype=np.uint64)
        assert other.lib.zc_ed_mul_gens(other.ctx, sets[2].id, v(K), v(out), 4) == ZC_ERR_BAD_ARG and err(other) == UNKNOWN
        g = other.generators(GR.generators(oracle, 3))                                   # left live: zc_ctx_destroy frees it
        assert np.array_equal(other.ris_mul_gens_compress(g, GR.scalars(3, 65)), GR.want(oracle, 3, 65)[1])
        g.id = 0
    finally:
        other.close()


# ------------------------------------------------------------------ argument checks
def test_no_rows_mixed_memory_and_the_order_of_the_checks(eng, sets):
    import torch
    lib, gid, count = eng.lib, sets[3].id, 3
    K = GR.scalars(count, 4)
    dK, out, out32 = dev(K), torch.full((4, 20), 0x6E, dtype=torch.int64, device="cuda"), torch.full((4, 32), 0xEE, dtype=torch.uint8, device="cuda")
    hout, hout32 = np.zeros((4, 20), dtype=np.uint64), np.zeros((4, 32), dtype=np.uint8)
    eng._follow_torch_stream(dK)
    assert lib.zc_ed_mul_gens(eng.ctx, gid, v(dK), v(out), 0) == 0 and lib.zc_ris_mul_gens_compress(eng.ctx, gid, v(dK), v(out32), 0) == 0
    assert lib.zc_ed_mul_gens(eng.ctx, gid, v(K), v(hout), 0) == 0
    torch.cuda.synchronize()
    assert (host(out) == 0x6E).all() and (host(out32) == 0xEE).all() and not hout.any()
    assert eng.ed_mul_gens(sets[3], np.zeros((0, count, 5), dtype=np.uint64)).shape == (0, 20)
    assert lib.zc_ed_mul_gens(eng.ctx, gid, v(dK), v(hout), 4) == ZC_ERR_MIXED_MEM
    assert lib.zc_ed_mul_gens(eng.ctx, gid, v(K), v(out), 4) == ZC_ERR_MIXED_MEM
    assert lib.zc_ris_mul_gens_compress(eng.ctx, gid, v(dK), v(hout32), 4) == ZC_ERR_MIXED_MEM
    assert lib.zc_ris_mul_gens_compress(eng.ctx, gid, v(K), v(out32), 4) == ZC_ERR_MIXED_MEM
    for name, o, oname in ((ED, hout, "out"), (RIS, hout32, "out32")):
        fn = getattr(lib, name)
        assert fn(eng.ctx, 0, None, v(o), 0) == ZC_ERR_BAD_ARG and err(eng) == "null pointer: scalars"      # the pointers before the id and n == 0
        assert fn(eng.ctx, 0, v(K), None, 0) == ZC_ERR_BAD_ARG and err(eng) == "null pointer: %s" % oname
        assert fn(eng.ctx, 0, v(K), v(o), 0) == ZC_ERR_BAD_ARG and err(eng) == UNKNOWN                        # the id before n == 0
        edge = -(-(1 << 31) // count)                                                                         # the first n with n * count >= 2^31
        assert fn(eng.ctx, gid, v(K), v(o), edge) == ZC_ERR_BAD_ARG and err(eng) == "%s: n * count must stay below 2^31" % name
        assert fn(eng.ctx, 0, v(K), v(o), edge) == ZC_ERR_BAD_ARG and err(eng) == UNKNOWN                     # the id before the limit
    torch.cuda.synchronize()
    assert (host(out) == 0x6E).all() and not hout.any() and not hout32.any()
