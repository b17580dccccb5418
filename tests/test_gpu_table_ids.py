"""GPU tier: the ids of the three kinds of context-owned tables -- fixed-base MSM tables (zc_msm_bases_*, zc_msm_fixed), generator
sets (zc_gens_*, zc_ed_mul_gens, zc_ris_mul_gens_compress) and baby-step tables (zc_dlog_*, zc_ed_dlog, zc_ris_dlog) -- through the
C ABI.  One engine holds one table of each kind at the smallest sizes that exist (4 bases, one generator, 2^4 baby steps plain
and with ZC_DLOG_COSET4).  Each of the eight calls that take an id refuses every id that is not a live table of its own kind in
its own context, with its own message and without touching its outputs; the tables answer as before afterwards; no two ids are
equal, whatever the kind; and a context closed with a live table of each kind gives all their device memory back."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from tests import dlog_rows as DR
from tests import gens_rows as GR
from tests import vectors as V

pytestmark = pytest.mark.gpu

ZC_ERR_BAD_ARG = -1
ROWS = 4
FILL = 0xA5
SLACK = 8 << 20                     # free-memory noise allowed across create / close cycles (as tests/test_gpu_ctx_lifecycle.py)
# call -> (the kind of id it takes, its message for an id that is no live table of that kind in this context)
CALLS = {
    "zc_msm_fixed": ("bases", "zc_msm_fixed: no live table of this context has this id"),
    "zc_msm_bases_destroy": ("bases", "zc_msm_bases_destroy: no live table of this context has this id"),
    "zc_ed_mul_gens": ("gens", "unknown generator set"),
    "zc_ris_mul_gens_compress": ("gens", "unknown generator set"),
    "zc_gens_destroy": ("gens", "unknown generator set"),
    "zc_ed_dlog": ("dlog", "unknown dlog table"),
    "zc_ris_dlog": ("dlog", "unknown dlog table"),
    "zc_dlog_destroy": ("dlog", "unknown dlog table"),
}


def v(x):
    return C.c_void_p(x.ctypes.data)


def one_of_each(e, oracle, w):
    """A table of each kind in e's context: kind -> handle ("dlog" plain, "coset" with ZC_DLOG_COSET4)."""
    t = {"bases": e.msm_bases(w.P), "gens": e.generators(GR.generators(oracle, 1)), "dlog": e.dlog_table(DR.generator(oracle, "B"), 4),
         "coset": e.dlog_table(DR.generator(oracle, "B"), 4, coset4=True)}
    w.ids += [h.id for h in t.values()]
    return t


@pytest.fixture(scope="module")
def world(oracle):
    """The engine under test with its four tables, one destroyed id of each kind, and a second engine with tables of its own."""
    import dusk_zerocaf_amd as z
    w = SimpleNamespace(ids=[], P=V.base_multiples(oracle, ROWS, V.SEED + 0x1D5))
    w.eng, w.other = z.Engine(), z.Engine()
    try:
        dead = one_of_each(w.eng, oracle, w)
        w.dead = {k: h.id for k, h in dead.items()}
        for h in dead.values():
            h.close()
        w.live = one_of_each(w.eng, oracle, w)
        w.foreign = one_of_each(w.other, oracle, w)
        yield w
        for h in w.live.values():
            h.close()
        for h in w.foreign.values():                # left live: the context's close takes them along
            h.id = 0
    finally:
        w.other.close()
        w.eng.close()


def kind_of(key):
    return "dlog" if key == "coset" else key


@pytest.mark.parametrize("name", list(CALLS))
def test_an_id_that_is_no_live_table_of_the_calls_kind_is_refused(world, oracle, name):
    w, lib, ctx = world, world.eng.lib, world.eng.ctx
    kind, message = CALLS[name]
    K1, K4 = np.ascontiguousarray(GR.scalars(1, ROWS)), np.ascontiguousarray(GR.scalars(ROWS, ROWS))
    p4 = np.ascontiguousarray(DR.ed_rows(oracle, "B", 4, 0)["points"][1:1 + ROWS])
    e4 = np.ascontiguousarray(DR.wire_rows(oracle, "B", 4)["enc"][1:1 + ROWS])
    pts, enc = np.full((ROWS, 20), FILL, dtype=np.uint64), np.full((ROWS, 32), FILL, dtype=np.uint8)
    m, found, ok = np.full(ROWS, FILL, dtype=np.uint64), np.full(ROWS, FILL, dtype=np.uint8), np.full(ROWS, FILL, dtype=np.uint8)
    call = {
        "zc_msm_fixed": lambda i: lib.zc_msm_fixed(ctx, i, v(K4), ROWS, v(pts)),
        "zc_msm_bases_destroy": lambda i: lib.zc_msm_bases_destroy(ctx, i),
        "zc_ed_mul_gens": lambda i: lib.zc_ed_mul_gens(ctx, i, v(K1), v(pts), ROWS),
        "zc_ris_mul_gens_compress": lambda i: lib.zc_ris_mul_gens_compress(ctx, i, v(K1), v(enc), ROWS),
        "zc_gens_destroy": lambda i: lib.zc_gens_destroy(ctx, i),
        "zc_ed_dlog": lambda i: lib.zc_ed_dlog(ctx, i, v(p4), 64, v(m), v(found), v(ok), ROWS),
        "zc_ris_dlog": lambda i: lib.zc_ris_dlog(ctx, i, v(e4), 64, v(m), v(found), v(ok), ROWS),
        "zc_dlog_destroy": lambda i: lib.zc_dlog_destroy(ctx, i),
    }[name]
    ids = [("live %s" % k, h.id) for k, h in w.live.items() if kind_of(k) != kind]
    ids += [("zero", 0), ("never issued", max(w.ids) + (1 << 40))]
    ids += [("destroyed %s" % k, i) for k, i in w.dead.items() if kind_of(k) == kind]
    ids += [("another context's %s" % k, h.id) for k, h in w.foreign.items()]
    assert len(ids) >= 6
    for what, i in ids:
        assert call(C.c_uint64(i)) == ZC_ERR_BAD_ARG, (name, what)
        assert lib.zc_last_error().decode() == message, (name, what)
    for out in (pts, enc, m, found, ok):
        assert (out == FILL).all(), name


def same_point(oracle, got, want):
    got, want = np.ascontiguousarray(got).reshape(-1, 20), np.ascontiguousarray(want).reshape(-1, 20)
    assert oracle.ed_eq(got, want).all()
    assert np.array_equal(oracle.ed_compress(got)[0], oracle.ed_compress(want)[0])
    assert np.array_equal(oracle.ris_compress(got), oracle.ris_compress(want))


def answers(e, t, oracle, P):
    """Four rows through every table of `t` against the oracle."""
    K = np.ascontiguousarray(V.rand_scalars_np(ROWS * len(P), V.SEED + 0x1D6, bits=252).reshape(ROWS, len(P), 5))
    K[1, 0] = 0
    got = t["bases"].msm(K)
    assert got.shape == (ROWS, 20)
    for b in range(ROWS):
        same_point(oracle, got[b], oracle.msm_naive(P, K[b]))
    pts, enc = GR.want(oracle, 1, ROWS)
    same_point(oracle, e.ed_mul_gens(t["gens"], GR.scalars(1, ROWS)), pts)
    assert np.array_equal(e.ris_mul_gens_compress(t["gens"], GR.scalars(1, ROWS)), enc)
    R, W = DR.ed_rows(oracle, "B", 4, 0), DR.wire_rows(oracle, "B", 4)
    assert R["found"][1:1 + ROWS].all() and W["found"][1:1 + ROWS].all()
    for key in ("dlog", "coset"):
        m, found, ok = t[key].ed(np.ascontiguousarray(R["points"][1:1 + ROWS]), 64)
        assert np.array_equal(m, R["m"][1:1 + ROWS]) and found.all() and ok.all()
    m, found, ok = t["coset"].ris(np.ascontiguousarray(W["enc"][1:1 + ROWS]), 64)
    assert np.array_equal(m, W["m"][1:1 + ROWS]) and found.all() and ok.all()


def test_the_tables_still_answer_after_the_refusals(world, oracle):
    answers(world.eng, world.live, oracle, world.P)
    answers(world.other, world.foreign, oracle, world.P)


def test_a_context_closed_with_a_live_table_of_each_kind_returns_their_memory(world, oracle):
    """Create / use / close cycles of a second engine that leaves a table of each kind live, by the method and the bound of
    test_context_cycles_return_all_device_memory: after the first cycle (which warms the runtime's own pools) free device
    memory stays within 8 MiB over nine more.  The tables left live hold at least 3 MiB each (1024 bases, eight generators,
    2^17 baby steps), so a single one that the close forgot would show; the four smallest tables are created, used and left
    live beside them."""
    import torch
    import dusk_zerocaf_amd as z
    big = V.base_multiples(oracle, 1024, V.SEED + 0x1D7)
    assert world.eng.msm_fixed_plan(1024)["table_mib"] >= 3 and 8 * GR.TABLE_WORDS * 4 >= 3 << 20 and (32 << 17) >= 3 << 20

    def cycle():
        e = z.Engine()
        try:
            t = one_of_each(e, oracle, world)
            t["big bases"], t["big gens"] = e.msm_bases(big), e.generators(GR.generators(oracle, 8))
            t["big dlog"] = e.dlog_table(DR.generator(oracle, "B"), 17)
            world.ids += [t[k].id for k in ("big bases", "big gens", "big dlog")]
            answers(e, t, oracle, world.P)
        finally:
            e.close()                               # with every table live
        for h in t.values():
            h.id = 0

    cycle()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(9):
        cycle()
    torch.cuda.synchronize()
    drift = torch.cuda.mem_get_info()[0] - free0
    print("free-memory drift over 9 cycles: %d bytes" % drift)
    assert abs(drift) < SLACK
    answers(world.eng, world.live, oracle, world.P)         # the first engine's tables are not touched by any of it


def test_all_ids_are_nonzero_and_pairwise_distinct_across_kinds(world):
    assert len(world.ids) >= 12 and 0 not in world.ids
    assert len(set(world.ids)) == len(world.ids)
