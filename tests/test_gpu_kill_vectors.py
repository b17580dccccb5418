"""GPU tier: the kill-vector families of tests/kill_vectors.py through the C ABI (Engine), bit for bit -- or as group elements
where the header promises only that (the windowed scalar multiplication, the linear combinations, mul_base).

The CPU tier (tests/test_mutants_emul.py) shows that these rows catch a wrong line in the headers' host build; here the same
rows meet the kernels in the launch forms that batches of at most 300 rows reach: the families as built and tiled to 1, 63,
65, 257 and 300 rows, host arrays, device tensors and host arrays that start 8 bytes off a 16-byte boundary, and for the shared
inversions ZC_INV_CHUNK = 2, 7, 64 next to the default one row per lane.  The worst-case inversion inputs fill their batches,
so every position of every chunk holds one.  At these sizes the strict scalar multiplication is always the four-lanes-per-row
kernel (k_ed_scalar_mul_quad), the point additions and the stand-alone products always run per lane, and the products' waves
are whatever 64 consecutive rows of a family happen to be.  The other forms -- the independent-chain, workgroup and
persistent-wave strict kernels and ZC_SCHED, the staged point and 40-byte kernels, and the products with their rows packed so
that whole waves take the one-pass or the two-pass form -- are in tests/test_gpu_kill_vector_forms.py.  Operations that exist
only in the emulation (digit strings, step counts, the interleaved multiplier) are left to the CPU tier."""
import pytest

from tests import kill_vectors as KV
from tests import vectors as V

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 65, 257, 300]
INVERSION_FAMILIES = ["field_core", "zero_by_value_p", "zero_by_value_l", "longest_inversions_p", "longest_inversions_l"]


@pytest.fixture(scope="module")
def eng():
    import dusk_zerocaf_amd as z
    e = z.Engine()
    yield e
    e.close()


def tiled(family, n, shift):
    return [c.tiled(n, shift) for c in KV.FAMILIES[family].cases() if c.rowwise]


@pytest.mark.parametrize("form", ["host", "device", "misaligned"])
@pytest.mark.parametrize("family", sorted(KV.FAMILIES))
def test_family_as_built(eng, family, form):
    backend = KV.EngineBackend(eng, device=form == "device", misalign=form == "misaligned")
    assert KV.run(family, backend) == []


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("family", sorted(KV.FAMILIES))
def test_family_at_batch_size(eng, family, n):
    """The rows repeated to n, starting n rows in: another part of every family lands in the one-row and the ragged launches."""
    assert KV.run(family, KV.EngineBackend(eng), tiled(family, n, n)) == []
    assert KV.run(family, KV.EngineBackend(eng, device=True), tiled(family, n, 3 * n + 1)) == []


@pytest.mark.parametrize("c", KV.INV_CHUNKS)
@pytest.mark.parametrize("family", INVERSION_FAMILIES)
def test_shared_inversions(family, c):
    """fe_invert / fe_div / ed_to_affine / sc_invert at c rows per lane: as built, and at every batch size from two offsets."""
    with V.tuned(ZC_INV_CHUNK=c) as te:
        assert KV.run(family, KV.EngineBackend(te, chunk=c)) == []
        for n in SIZES:
            for shift, device in ((0, False), (n + 1, True)):
                assert KV.run(family, KV.EngineBackend(te, chunk=c, device=device), tiled(family, n, shift)) == [], (n, shift)
