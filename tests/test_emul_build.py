"""CPU tier: tests/emul_build.py decides by itself when an emulation library is stale.  Every test works on a copied tree under
tmp_path (the headers and one emulation source), so nothing in the repository is touched or built."""
import os

import pytest

from tests import emul_build as EB

SOURCE = "ris_dac_emul.cpp"                          # includes zc_ris_batch.hip.h, which includes zc_msm_plan.h for ZC_BLOCK
MUTANT = dict(name="block_of_128", header="zc_msm_plan.h", old="constexpr int ZC_BLOCK = 256;", new="constexpr int ZC_BLOCK = 128;")


@pytest.fixture()
def tree(tmp_path):
    if not EB.have_rocm():
        pytest.skip("ROCm headers not present")
    return EB._mutated_copy(str(tmp_path / "tree"), [SOURCE], None, None)


def _stamp(path):
    return os.stat(path).st_mtime_ns


def test_library_names():
    assert EB.library_name("emul.cpp", sanitize=True) == "libzc_emul_san.so"              # the name tests/test_sanitizers.py waits for
    assert EB.library_name("sm_tile_emul.cpp", checked=True, sanitize=True) == "libzc_sm_tile_san_checked.so"
    assert EB.library_name("ris_dac_emul.cpp", checked=True) == "libzc_ris_dac_checked.so"


def test_an_included_header_two_levels_down_makes_the_library_stale(tree):
    so = EB.library(SOURCE, root=tree)
    assert so.startswith(tree + os.sep)
    with open(so + ".dep") as f:
        deps = f.read().split("\n")[1:]
    assert os.path.join(tree, "dusk_zerocaf_amd", "csrc", "zc_msm_plan.h") in [os.path.normpath(d) for d in deps]
    before = _stamp(so)
    assert EB.library(SOURCE, root=tree) == so and _stamp(so) == before                   # nothing touched: nothing rebuilt
    later = os.path.getmtime(so) + 50
    os.utime(os.path.join(tree, "dusk_zerocaf_amd", "csrc", "zc_msm_plan.h"), (later, later))       # newer than the library
    assert EB.library(SOURCE, root=tree) == so and _stamp(so) > before


def test_another_flag_set_rebuilds(tree):
    so = EB.library(SOURCE, root=tree)
    before = _stamp(so)
    assert EB.library(SOURCE, root=tree, flags=("-DZC_SOME_KNOB=1",)) == so and _stamp(so) > before
    before = _stamp(so)
    assert EB.library(SOURCE, root=tree, flags=("-DZC_SOME_KNOB=1",)) == so and _stamp(so) == before
    assert EB.library(SOURCE, root=tree, checked=True) != so                              # a variant is another file, not a rebuild


def test_mutant_builds_write_nothing_into_the_repository(tmp_path_factory):
    def snapshot():
        return {(d, f, os.path.getmtime(os.path.join(d, f))) for top in ("tests", "dusk_zerocaf_amd")
                for d, _, files in os.walk(os.path.join(EB.ROOT, top)) if "__pycache__" not in d for f in files}
    before = snapshot()
    built = EB.mutant_builds(tmp_path_factory, [MUTANT], SOURCE, workers=2)
    assert snapshot() == before
    assert set(built) == {None, "block_of_128"} and all(os.path.exists(p) and not p.startswith(EB.ROOT + os.sep) for p in built.values())
    text = lambda so: open(os.path.join(os.path.dirname(so), "..", "..", "dusk_zerocaf_amd", "csrc", MUTANT["header"])).read()
    assert MUTANT["new"] in text(built["block_of_128"]) and MUTANT["old"] in text(built[None])
    with pytest.raises(AssertionError):
        EB.catalogue_is_sound([MUTANT, MUTANT])                                           # a name twice
    EB.catalogue_is_sound([MUTANT])
