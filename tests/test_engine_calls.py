"""CPU tier: what every public Engine / MsmBases method hands to the C ABI -- symbol, argument order, which pointer is which
array, by-value arguments -- and the kind, dtype and shape of what it returns, for numpy arrays and for torch tensors, against
the table recorded before the methods were rewritten on one shared description (tests/golden/gen_engine_calls.py; the library
is a recording stand-in, as in tests/test_abi.py: nothing is computed)."""
import importlib.util
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gen():
    spec = importlib.util.spec_from_file_location("gen_engine_calls", os.path.join(ROOT, "tests", "golden", "gen_engine_calls.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def test_every_public_method_is_covered():
    from dusk_zerocaf_amd import engine
    gen = _gen()
    assert gen.public_methods(engine) - gen.LEFT_OUT == gen.covered()


def test_calls_and_results_match_the_recorded_table():
    from dusk_zerocaf_amd import engine
    gen = _gen()
    with open(gen.OUT) as f:
        want = json.load(f)
    got = json.loads(json.dumps(gen.observe(engine)))          # tuples -> lists, as the file has them
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        assert got[key] == want[key], key


# every method that takes two or more row arrays: (method, (width, dtype) per array, extra keyword arguments)
MULTI = [(pre + op, [(w, np.uint64)] * 2, {}) for pre, w in (("fe_", 5), ("sc_", 5)) for op in ("add", "sub", "mul", "pow")] + \
        [(pre + op, [(w, np.uint64)] * 2, {}) for pre, w in (("ed_", 20), ("proj_", 15)) for op in ("add", "sub")] + \
        [("fe_div", [(5, np.uint64)] * 2, {}), ("fe_sqrt_ratio_i", [(5, np.uint64)] * 2, {}),
         ("ed_eq", [(20, np.uint64)] * 2, {}), ("ris_eq", [(20, np.uint64)] * 2, {}), ("proj_eq", [(15, np.uint64)] * 2, {}),
         ("ed_scalar_mul", [(20, np.uint64), (5, np.uint64)], {}), ("ed_scalar_mul", [(20, np.uint64), (5, np.uint64), (20, np.uint64)], {}),
         ("proj_scalar_mul", [(15, np.uint64), (5, np.uint64)], {}),
         ("ris_roundtrip_mul", [(32, np.uint8), (5, np.uint64)], {}), ("ris_roundtrip_mul", [(32, np.uint8), (5, np.uint64), (32, np.uint8)], {}),
         ("msm", [(20, np.uint64), (5, np.uint64)], {}), ("msm_sharded", [(20, np.uint64), (5, np.uint64)], {}),
         ("msm_partial", [(20, np.uint64), (5, np.uint64)], {"out": "tensor"}),
         ("ed_lincomb", [(2, 20, np.uint64), (2, 5, np.uint64)], {}), ("msm_batch", [(2, 20, np.uint64), (2, 5, np.uint64)], {}),
         ("ris_lincomb", [(2, 32, np.uint8), (2, 5, np.uint64)], {}), ("ris_lincomb", [(2, 32, np.uint8), (2, 5, np.uint64), (5, np.uint64)], {})]


@pytest.mark.parametrize("case", range(len(MULTI)), ids=["%s-%d" % (m[0], len(m[1])) for m in MULTI])
def test_unequal_row_counts_are_refused_before_the_library_is_called(case):
    """The library reads n rows of every array: an array with fewer rows than the first would be read past its end."""
    from dusk_zerocaf_amd import engine
    name, specs, kw = MULTI[case]
    if kw.get("out") == "tensor":
        import torch
        kw = {"out": torch.zeros((1, 20), dtype=torch.int64)}
    make = lambda n, spec: np.zeros((n,) + tuple(spec[:-1]), dtype=spec[-1])
    e, rec = _gen().new_engine(engine)
    try:
        getattr(e, name)(*[make(3, s) for s in specs], **kw)   # equal counts: the call goes through
        assert len(rec.calls) == 1
        for short in range(1, len(specs)):                     # then each later array in turn with another count
            for n in (2, 4):
                with pytest.raises(AssertionError):
                    getattr(e, name)(*[make(n if i == short else 3, s) for i, s in enumerate(specs)], **kw)
        assert len(rec.calls) == 1
    finally:
        e.ctx = None
