"""CPU tier: the wave model behind the packed `mulmod` kill vectors.

The stand-alone products choose their form per wave on the device (zc_arith.hip.h: mulsq_wave_any is a ballot): one operand
at or above 2^TOPBIT sends all 64 rows of its wave through the two Montgomery passes.  The emulation decides per row, so a row
proven to kill a defect of the one-pass product proves nothing on the GPU unless its whole wave is eligible -- and a row that
should meet the two-pass product must share a wave with an ineligible one.  Neither form can be observed from outside the
kernel; this model is the evidence that the packed batches of tests/test_gpu_kill_vector_forms.py take the form they name.

The model: a wave is 64 consecutive rows of one call.  That holds for the per-lane kernels (row = blockIdx * 256 + threadIdx)
and for the staged ones (elementwise_body: a workgroup stages rows [256 b, 256 b + 256) and thread t computes row 256 b + t);
rows past the end of the batch are inactive lanes and take no part in the ballot."""
import numpy as np
import pytest

from tests import kill_vectors as KV

TILED_SIZES = (1, 63, 65, 257, 300)              # tests/test_gpu_kill_vectors.py: SIZES, at shifts n and 3 n + 1


def mulmod_cases():
    return [c for c in KV.FAMILIES["field_core"].cases() if c.op == "mulmod"]


@pytest.mark.parametrize("which", ["mul", "sq"])
@pytest.mark.parametrize("modl", [0, 1])
def test_packings_fix_the_product_form(modl, which):
    case = mulmod_cases()[modl]
    assert case.params["modl"] == modl
    lv = KV.mulmod_levels(case, which)
    assert (lv == 0).sum() >= 64 and all((lv == k).any() for k in range(1, KV.MAX_LEVEL + 1))
    one, order = KV.packed(case, which, "one-pass")
    assert set(order.tolist()) == set(range(len(lv))) and np.array_equal(KV.mulmod_levels(one, which), lv[order])
    wl = KV.wave_levels(lv[order])
    assert (wl[lv[order] == 0] == 0).all()                       # every eligible row in an all-eligible wave
    assert (wl == lv[order]).all() and len(order) % KV.WAVE == 0   # and every other wave holds rows of one level only, no ragged wave
    assert all(np.array_equal(w[order], p) for w, p in zip(case.want, one.want))
    two, order = KV.packed(case, which, "two-pass")
    assert set(order.tolist()) == set(range(len(lv))) and np.array_equal(KV.mulmod_levels(two, which), lv[order])
    assert (KV.wave_levels(lv[order])[lv[order] == 0] > 0).all()   # every eligible row beside an ineligible one
    assert all(np.array_equal(w[order], p) for w, p in zip(case.want, two.want))


def test_what_the_plain_tilings_left_out():
    """The record of the gap: over the forms tests/test_gpu_kill_vectors.py uses -- the case as built, then 1, 63, 65, 257 and
    300 rows from row n and from row 3 n + 1 -- 59 of the 216 eligible pairs and 73 of the 317 eligible squares never sit in
    an all-eligible wave, mod p and mod L alike (mod - 1 at row 3 keeps the edge operands of the first wave on two passes)."""
    for case in mulmod_cases():
        for which, never, eligible in (("mul", 59, 216), ("sq", 73, 317)):
            lv = KV.mulmod_levels(case, which)
            n = len(lv)
            seen = np.zeros(n, dtype=bool)
            for order in [np.arange(n)] + [(np.arange(m) + shift) % n for m in TILED_SIZES for shift in (m, 3 * m + 1)]:
                seen[order[KV.wave_levels(lv[order]) == 0]] = True
            assert (int((lv == 0).sum()), int(((lv == 0) & ~seen).sum())) == (eligible, never), (case.label(), which)


def test_bad_rows_follows_mismatches():
    """Case.bad_rows: the rows behind `mismatches` -- exact limbs, the accept flag's masking, points compared as group elements."""
    a = KV.rows([1, 2, 3, 4])
    case = KV.Case("fe_half", [a], [a])
    got = a.copy()
    got[2, 0] ^= 1
    assert case.mismatches([got]) == [0] and case.bad_rows([got]) == [2] and case.bad_rows([a]) == []
    ok = KV.flags([1, 0, 1, 1])
    case = KV.Case("fe_invert", [a], [a, ok], ok=1)
    got = a.copy()
    got[1, 0] ^= 1                                               # a rejected row: only its flag is compared
    assert case.mismatches([got, ok]) == [] and case.bad_rows([got, ok]) == []
    got[3, 4] ^= 1
    assert case.bad_rows([got, ok]) == [3] and case.bad_rows([got, KV.flags([1, 1, 1, 1])]) == [1, 3]
    assert case.bad_rows([got, KV.flags([1, 1, 1, 1])], output=1) == [1]
    pts = KV.some_points(3, KV.SEED + 7)
    case = KV.Case("ed_mul_base", [a[:3]], [KV.affine_of(pts)], cmp="group")
    other = [KV.scaled(q, 5) for q in pts]                       # the same group elements in other coordinates
    assert case.bad_rows([KV.pt_rows(other)]) == []
    other[1] = pts[0]
    assert case.bad_rows([KV.pt_rows(other)]) == [1] and case.mismatches([KV.pt_rows(other)]) == [0]
