"""CPU tier: which pointers of every batched entry point are required, and the message that names a missing one.  The library
loads without a GPU and checks its pointers before it touches the context, so the calls are made with ctx = NULL; the table was
recorded before the entry points were rewritten on one typed buffer description (tests/golden/gen_null_contract.py)."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import dusk_zerocaf_amd as z
    if not os.path.exists(z.LIB_PATH):
        from dusk_zerocaf_amd import build
        build.build(test_hooks=True)
    return z.load()


def _gen():
    spec = importlib.util.spec_from_file_location("gen_null_contract", os.path.join(ROOT, "tests", "golden", "gen_null_contract.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def test_the_table_covers_every_batched_entry_point():
    from dusk_zerocaf_amd import _lib
    gen = _gen()
    with open(gen.OUT) as f:
        want = json.load(f)
    syms = gen.batched_symbols(_lib.SIGNATURES)
    assert len(syms) == 61 and sorted({k.split("{")[0] for k in want}) == sorted(syms)
    # what is left out has its own pipeline: the MSM family, the exchange step, the context calls
    assert sorted(set(_lib.SIGNATURES) - set(syms)) == ["zc_comm_destroy", "zc_comm_init", "zc_comm_size", "zc_ctx_set_stream_dev", "zc_ed_fold_ordered",
                                                        "zc_msm", "zc_msm_bases_create", "zc_msm_bases_destroy", "zc_msm_batch", "zc_msm_batch_plan",
                                                        "zc_msm_fixed", "zc_msm_fixed_plan", "zc_msm_partial", "zc_msm_plan", "zc_msm_sharded"]


def test_required_pointers_and_their_names(lib):
    from dusk_zerocaf_amd import _lib
    gen = _gen()
    with open(gen.OUT) as f:
        want = json.load(f)
    got = gen.observe(lib, _lib.SIGNATURES)
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        assert got[key] == want[key], key
