"""GPU tier: the kill vectors in the launch forms tests/test_gpu_kill_vectors.py cannot reach at its 300 rows.

An operation with several kernels picks one by batch size, by a ZC_* knob of the context, by the alignment of its arrays --
and, inside the stand-alone products, by a ballot over the wave.  The rows of tests/kill_vectors.py that the CPU tier proves
to kill planted defects are tiled (Case.tiled: expected rows come along, no oracle run) to the smallest batch that reaches
each form, on device tensors, so that one call is one launch of the kernel named here (proven by the test build's counters, which
count every answer of zc_launch_plan.h where the host code consumes it):

  strict scalar multiplication (group_core and recoding_fast `strict` -- and `small` where the form is that kernel -- and the
  rowwise recoding_tile cases, the two tiles the doubling gate must refuse among them)
      k_ed_scalar_mul_small          independent column chains            2^14 + 1 rows     (form counter)
      k_ed_scalar_mul                one workgroup per 256 rows           2^16 + 1
      k_ed_scalar_mul_pw             persistent waves                     2^17 + 77
      k_ed_scalar_mul_pw_unified     ZC_SCHED=unified                     2^17 + 77
      k_ed_scalar_mul                ZC_SCHED=block at that size          2^17 + 77
  ed_add_plain: add, sub, double (group_core)
      k_ed_*_staged                  staged 160-byte records              4097 rows, 16-byte aligned   (launch counter)
      k_ed_*                         per lane                             4097 rows, 8 bytes off       (launch counter)
  mulmod: product and square, mod p and mod L (field_core), each in the one-pass and the two-pass packing
      k_*_mul / k_*_square           per lane                             the packed case              (launch counter)
      k_*_stream                     staged, ZC_TEST_STREAM_MIN_BYTES=1   the same                     (launch counter)
      k_*_mul / k_*_square           that knob, rows 8 bytes off: the fall-back to per lane            (launch counter)

Which product form a wave takes cannot be seen from outside; tests/test_kill_vector_waves.py shows on the wave model that the
one-pass packing puts every eligible row into an all-eligible wave and the two-pass packing none.  Lanes and rows in the
staged 40-byte kernels (zc_kernels.hip.h: elementwise_body): workgroup b moves rows [256 b, 256 b + 256) through LDS with
cooperative 16-byte copies, then thread t computes row 256 b + t from its own LDS slot -- wave w of the workgroup holds the 64
consecutive rows 256 b + 64 w ..., as in the per-lane kernels, and threads past the end of the batch skip the product (they
are inactive in the ballot).  So the packings need no other order there.

Tile composition in the persistent kernels follows the cost sort and its atomics and is not controlled here: mixed tiles stay
with tests/test_gpu_scalar_mul_dg.py and tests/test_gpu_point_classes.py."""
import contextlib
import time

import pytest

from tests import entry_table as T
from tests import kill_vectors as KV
from tests import vectors as V

pytestmark = pytest.mark.gpu

PW_ROWS = T.PW_MIN_ELEMS + 77
STRICT_FORMS = {f.name: (f, n) for f, n in (
    (KV.Form("independent-chain kernel", KV.STRICT_OPS, lo=T.QUAD_LAUNCH_ELEMS + 1, hi=T.STRICT_SMALL_MAX_ELEMS, small=True, hooks=True, launch="strict_small"),
     T.QUAD_LAUNCH_ELEMS + 1),
    (KV.Form("one workgroup per 256 rows", KV.STRICT_OPS, lo=T.STRICT_SMALL_MAX_ELEMS + 1, hi=T.PW_MIN_ELEMS - 1, hooks=True, launch="strict_block"), T.STRICT_SMALL_MAX_ELEMS + 1),
    (KV.Form("persistent waves", KV.STRICT_OPS, lo=T.PW_MIN_ELEMS, hooks=True, launch="strict_pw"), PW_ROWS),
    (KV.Form("persistent waves, ZC_SCHED=unified", KV.STRICT_OPS, lo=T.PW_MIN_ELEMS, env={"ZC_SCHED": "unified"}, hooks=True, launch="strict_pw_unified"), PW_ROWS),
    (KV.Form("ZC_SCHED=block at the persistent size", KV.STRICT_OPS, lo=T.PW_MIN_ELEMS, env={"ZC_SCHED": "block"}, hooks=True, launch="strict_block"), PW_ROWS),
)}
STRICT_FAMILIES = ("group_core", "recoding_fast", "recoding_tile")
POINT_ROWS = T.ED_STAGED_MIN_POINTS + 1
POINT_FORMS = {f.name: f for f in (
    KV.Form("staged records", ("ed_add_plain",), lo=T.ED_STAGED_MIN_POINTS + 1, hooks=True, staged=True),
    KV.Form("per lane, rows 8 bytes off", ("ed_add_plain",), lo=T.ED_STAGED_MIN_POINTS + 1, hooks=True, staged=False, misalign=True),
)}
STREAM = {"ZC_TEST_STREAM_MIN_BYTES": 1}
PRODUCT_FORMS = {f.name: f for f in (
    KV.Form("per lane", ("mulmod",), hooks=True, staged=False),
    KV.Form("staged", ("mulmod",), env=STREAM, hooks=True, staged=True),
    KV.Form("staged knob, rows 8 bytes off: per lane", ("mulmod",), env=STREAM, hooks=True, staged=False, misalign=True),
)}
LAUNCHES = {"ed_add_plain": 1, "mulmod": 2}                  # kernels per case: mulmod is the product and the square


@pytest.fixture(scope="module")
def engines():
    """form -> an Engine whose context was created under the form's knobs, one per distinct setting, closed together."""
    with contextlib.ExitStack() as stack:
        made = {}

        def get(form):
            key = (form.hooks, tuple(sorted(form.env.items())))
            if key not in made:
                made[key] = stack.enter_context(V.tuned(hooks=form.hooks, **form.env))
            return made[key]
        yield get


@pytest.fixture(scope="module")
def families():
    """The cases of the families used here, built once (their expected rows are Python-integer arithmetic) and shared."""
    return {fam: KV.FAMILIES[fam].cases() for fam in STRICT_FAMILIES + ("field_core",)}


def run_form(backend, cases):
    """Every row of every case the form applies to must be the family's; returns the number of cases that ran."""
    made = 0
    for case in cases:
        got = backend.call(case)
        if got is None:
            continue
        made += 1
        bad = case.bad_rows(got)
        assert not bad, "%s in the form '%s': %d of %d rows differ from the family's, the first at %s" % (
            case.label(), backend.form.name, len(bad), len(case.ins[0]), bad[:8])
    assert made > 0, "the form '%s' ran nothing" % backend.form.name
    return made


def assert_counted(backend):
    """The test build's launch counter: every kernel of every call took the staged form, or none did."""
    assert backend.counted and all(c == (LAUNCHES[op] if backend.form.staged else 0) for op, c in backend.counted), (backend.form.name, backend.counted)


@pytest.mark.parametrize("name", list(STRICT_FORMS))
def test_strict_scalar_mul_forms(engines, families, name):
    form, n = STRICT_FORMS[name]
    t0 = time.perf_counter()
    backend = KV.EngineBackend(engines(form), form=form)
    cases = [c.tiled(n) for fam in STRICT_FAMILIES for c in families[fam] if c.rowwise and backend.takes(c)]
    made = run_form(backend, cases)
    assert made == (7 if form.small else 5), made                 # strict (+ small) of two families, the three rowwise tile cases
    # the test build's form counters: every call was exactly one launch, of the form this row names
    assert len(backend.forms) == made and all(delta == {form.launch: 1} for _, delta in backend.forms), (name, backend.forms)
    print("strict scalar-mul, %s: %d cases at n = %d%s (form counter: %s), %.2f s"
          % (name, made, n, "".join(" and %s=%s" % kv for kv in form.env.items()), [delta for _, delta in backend.forms], time.perf_counter() - t0))


@pytest.mark.parametrize("name", list(POINT_FORMS))
def test_point_addition_forms(engines, families, name):
    form = POINT_FORMS[name]
    t0 = time.perf_counter()
    backend = KV.EngineBackend(engines(form), form=form)
    made = run_form(backend, [c.tiled(POINT_ROWS) for c in families["group_core"] if c.rowwise and backend.takes(c)])
    assert made == 3, made                                       # add, sub, double
    assert_counted(backend)
    print("ed add / sub / double, %s: n = %d (launch counter: %s), %.2f s" % (name, POINT_ROWS, backend.counted, time.perf_counter() - t0))


@pytest.mark.parametrize("packing", ["one-pass", "two-pass"])
@pytest.mark.parametrize("name", list(PRODUCT_FORMS))
def test_product_forms(engines, families, name, packing):
    form = PRODUCT_FORMS[name]
    t0 = time.perf_counter()
    backend = KV.EngineBackend(engines(form), form=form)
    cases = [KV.packed(c, which, packing)[0] for c in families["field_core"] if c.op == "mulmod" for which in ("mul", "sq")]
    made = run_form(backend, cases)
    assert made == 4, made                                       # mod p and mod L, packed for the product and for the square
    assert_counted(backend)
    print("mul / square mod p and mod L, %s, %s packing (wave model: tests/test_kill_vector_waves.py): n = %s (launch counter: %s), %.2f s"
          % (name, packing, [len(c.ins[0]) for c in cases], backend.counted, time.perf_counter() - t0))
