"""GPU tier: zc_ris_lincomb_sum, out32 = compress(b * B + sum over the accepted rows of w_ij * decompress(in32[i][j])), through
the C ABI and the Engine, on host arrays and on device tensors.

Expected bytes: oracle.ris_compress(oracle.msm_naive_mt(points, w)) over the decodable rows, with the canonical w_ij and b
computed on Python integers (tests/ris_sum_rows.py); the smallest case also against oracle/pymodel.py alone.  Every byte and
every flag is compared.  The shapes are the smallest at which each part can go wrong: one and two pairs, 4095 / 4096 / 4097
pairs around the MSM's bucket threshold, the bucket regime with 1, 2 and 7 terms (7 does not divide 8192: 1171 rows, 8198
pairs), n = 63, 64, 65, 257 for the first stage of the base term's reduction, and one more row than a workgroup of k_sc_sum's
first launch covers, read from the kernel's constants."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

from oracle import pymodel as pm
from tests import framed_buffers as FB
from tests import ris_lincomb_rows as RR
from tests import ris_sum_rows as RS
from tests import scalar_ext_rows as SX
from tests import vectors as V

pytestmark = pytest.mark.gpu

ZC_OK, ZC_ERR_BAD_ARG, ZC_ERR_MIXED_MEM = 0, -1, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dusk_zerocaf_amd", "csrc")
SEED = V.SEED + 0x5B00
L = pm.L
VP = C.c_void_p


def _constant(header, name):
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([0-9 <]+);" % name, open(os.path.join(CSRC, header)).read())
    assert m, name
    return int(eval(m.group(1)))


SUM_SPAN = _constant("zc_msm_plan.h", "ZC_BLOCK") * _constant("zc_ris_batch.hip.h", "SC_SUM_ROWS_PER_LANE")   # rows per workgroup of the first launch
BUCKET_MIN = _constant("zc_msm_plan.h", "MSM_BUCKET_MIN_N")


@pytest.fixture(scope="module")
def eng():
    import dusk_zerocaf_amd as z
    e = z.Engine()
    yield e
    e.close()


def to_dev(a):
    import torch
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.dtype == np.uint8 else a.view(np.int64)).cuda()


def to_host(t):
    a = t.cpu().numpy()
    return a if a.dtype == np.uint8 else a.view(np.uint64)


def _p(a):
    return None if a is None else VP(a.ctypes.data)


def abi(eng, E, K, KB=None, Z=None, want_ok=True):
    """The C call on host arrays: (rc, 32 bytes, ok or None); out32 and ok framed with 0xA5."""
    E, K = np.ascontiguousarray(E, dtype=np.uint8), np.ascontiguousarray(K, dtype=np.uint64)
    n, t = E.shape[:2]
    out = np.full(96, 0xA5, dtype=np.uint8)
    ok = np.full(n + 64, 0xA5, dtype=np.uint8)
    rc = eng.lib.zc_ris_lincomb_sum(eng.ctx, _p(E), _p(K), t, _p(KB), _p(Z), VP(out.ctypes.data + 32), VP(ok.ctypes.data + 32) if want_ok else None, n)
    assert (out[:32] == 0xA5).all() and (out[64:] == 0xA5).all() and (ok[:32] == 0xA5).all() and (ok[32 + n:] == 0xA5).all()
    if not want_ok:
        assert (ok == 0xA5).all()
    return rc, bytes(out[32:64]), (ok[32:32 + n].copy() if want_ok else None)


def both_placements(eng, E, K, KB=None, Z=None):
    """Host arrays through the C ABI and device tensors through the Engine: identical; returns (bytes, ok)."""
    rc, got, ok = abi(eng, E, K, KB, Z)
    assert rc == ZC_OK, eng.lib.zc_last_error()
    dgot, dok = eng.ris_lincomb_sum(to_dev(E), to_dev(K), to_dev(KB), to_dev(Z))
    assert dok.is_cuda and isinstance(dgot, bytes)
    assert dgot == got and np.array_equal(to_host(dok), ok)
    return got, ok


def batch(oracle, n, t, seed, reject=True, canonical=False):
    E = RS.encodings_of_multiples(oracle, n * t, seed).reshape(n, t, 32)
    rows = RS.plant_rejected(oracle, E, seed + 1) if reject else []
    mk = RS.canonical_scalars if canonical else RS.mixed_scalars
    return E, mk(n * t, seed + 2).reshape(n, t, 5), mk(n, seed + 3), mk(n, seed + 4), rows


# (n, terms, base term): pairs = n terms (+ 1)
SHAPES = [(1, 1, False), (1, 1, True),
          (BUCKET_MIN - 1, 1, False), (BUCKET_MIN - 1, 1, True), (BUCKET_MIN, 1, True), (BUCKET_MIN // 2, 2, False),
          (8192, 1, True), (4096, 2, True), (1171, 7, True),
          (63, 2, True), (64, 2, True), (65, 2, True), (257, 2, True),
          (SUM_SPAN + 1, 1, True)]


@pytest.mark.parametrize("n,t,base", SHAPES, ids=["%dx%d%s" % (n, t, "+B" if b else "") for n, t, b in SHAPES])
def test_shapes_vs_oracle_on_host_arrays_and_device_tensors(eng, oracle, n, t, base):
    """Weights and scalars canonical, zero, L - 1, 128-bit and raw patterns at or above L; encodings of k B, the identity, the
    sixteen [0..15] B, one public key in many rows; an undecodable term in every 17th row and in the first and the last."""
    assert (BUCKET_MIN - 1, BUCKET_MIN, BUCKET_MIN + 1) == (4095, 4096, 4097) and SUM_SPAN + 1 == 1025
    E, K, KB, Z, rejected = batch(oracle, n, t, SEED + 31 * n + t)
    KB = KB if base else None
    want, wok = RS.expected(oracle, E, K, KB, Z)
    got, ok = both_placements(eng, E, K, KB, Z)
    assert np.array_equal(ok, wok) and sorted(np.flatnonzero(ok == 0)) == rejected
    assert got == want
    assert n < 3 or want != RS.ZERO32


def test_smallest_case_against_the_python_model_alone(eng):
    n, t = 3, 2
    E = np.array([list(pm.ris_compress(pm.ed_scalar_mul(pm.BASEPOINT, 7 * i + 3))) for i in range(n * t)], dtype=np.uint8).reshape(n, t, 32)
    K, KB, Z = RS.mixed_scalars(n * t, SEED + 1).reshape(n, t, 5), RS.mixed_scalars(n, SEED + 2), RS.weights128(n, SEED + 3)
    for KBx, Zx in ((KB, Z), (None, Z), (KB, None), (None, None)):
        want, wok = RS.expected_pymodel(E, K, KBx, Zx)
        got, ok = both_placements(eng, E, K, KBx, Zx)
        assert got == want and ok.tolist() == wok.tolist() == [1, 1, 1]
    E[1, 1] = RR.le32(pm.P + 1)
    want, wok = RS.expected_pymodel(E, K, KB, Z)
    got, ok = both_placements(eng, E, K, KB, Z)
    assert got == want and ok.tolist() == wok.tolist() == [1, 0, 1]


@pytest.mark.parametrize("n,t", [(40, 2), (BUCKET_MIN + 100, 1)])
def test_a_batch_of_only_rejected_rows_gives_zero_bytes(eng, oracle, n, t):
    E, K, KB, Z, _ = batch(oracle, n, t, SEED + 50 + n, reject=False)
    bad = RS.bad_encodings(oracle, E[0, 0], SEED + 51)
    for i in range(n):
        E[i, i % t] = bad[i % len(bad)]
    got, ok = both_placements(eng, E, K, KB, Z)
    assert got == RS.ZERO32 and not ok.any()
    got, ok = both_placements(eng, E, K, None, None)
    assert got == RS.ZERO32 and not ok.any()


def test_equal_and_opposite_points_meet_and_cancel(eng, oracle):
    """Rows [P_i, -P_i]: with equal scalars the sum is the identity (32 zero bytes); with different ones the oracle's bytes.  2048
    rows of two terms: the bucket regime, where P and -P land in one bucket."""
    n = BUCKET_MIN // 2
    P = V.base_multiples(oracle, n, SEED + 60)
    E = np.stack([oracle.ris_compress(P), oracle.ris_compress(eng.ed_neg(P))], axis=1)
    K = RS.canonical_scalars(n, SEED + 61).reshape(n, 1, 5).repeat(2, axis=1)
    Z = RS.weights128(n, SEED + 62)
    got, ok = both_placements(eng, E, K, None, Z)
    assert got == RS.ZERO32 and ok.all()
    K2 = np.ascontiguousarray(K)
    K2[:, 1] = RS.canonical_scalars(n, SEED + 63)
    got, ok = both_placements(eng, E, K2, None, Z)
    assert got == RS.expected(oracle, E, K2, None, Z)[0] != RS.ZERO32 and ok.all()


@pytest.mark.parametrize("n,t", [(50, 2), (BUCKET_MIN + 104, 1)])
def test_a_rejected_row_takes_only_itself_out(eng, oracle, n, t):
    """One accepted row replaced by a rejected one, whatever its scalars and weight: the bytes are exactly the oracle's sum
    without that row."""
    E, K, KB, Z, rejected = batch(oracle, n, t, SEED + 70 + n)
    base, _ = both_placements(eng, E, K, KB, Z)
    assert base == RS.expected(oracle, E, K, KB, Z)[0]
    for r, pat in ((n // 2 + 1, pm.limbs(L - 1)), (1, [SX.ALL_ONES] * 5), (n - 3, [0] * 5)):
        assert r not in rejected
        E2, K2, KB2, Z2 = E.copy(), K.copy(), KB.copy(), Z.copy()
        E2[r, t - 1] = RS.bad_encodings(oracle, E[r, t - 1], SEED + 71 + r)[r % 4]
        K2[r], KB2[r], Z2[r] = pat, pat, pat
        got, ok = both_placements(eng, E2, K2, KB2, Z2)
        keep = np.arange(n) != r
        without, wok = RS.expected(oracle, E[keep], K[keep], KB[keep], Z[keep])
        assert got == without and got != base
        assert ok[r] == 0 and np.array_equal(ok[keep], wok)


def test_schnorr_batch_verification(eng, oracle):
    """1024 rows R = r B, A = a B, s = r + c a: terms [A, L - c] and [R, L - 1], base s, random 128-bit weights: every ok is 1
    and the sum is the identity.  With one s altered the bytes are nonzero and the oracle's."""
    n = 1024
    rng = random.Random(SEED + 80)
    r, a, c = ([rng.randrange(1, L) for _ in range(n)] for _ in range(3))
    s = [(ri + ci * ai) % L for ri, ai, ci in zip(r, a, c)]
    B = RR.basepoint_rows(n)
    enc = lambda ks: oracle.mt(oracle.ris_compress, oracle.mt(oracle.ed_scalar_mul, B, SX.rows(ks)))
    E = np.stack([enc(a), enc(r)], axis=1)
    K = np.stack([SX.rows([L - ci for ci in c]), SX.rows([L - 1] * n)], axis=1)
    KB, Z = SX.rows(s), RS.weights128(n, SEED + 81)
    got, ok = both_placements(eng, E, K, KB, Z)
    assert ok.all() and got == RS.ZERO32
    KB[517] = pm.limbs((s[517] + 1) % L)
    got, ok = both_placements(eng, E, K, KB, Z)
    assert ok.all() and got != RS.ZERO32 and got == RS.expected(oracle, E, K, KB, Z)[0]


@pytest.mark.parametrize("n", [100, BUCKET_MIN + 904])
def test_without_weights_and_base_it_is_the_msm_over_the_decoded_points(eng, oracle, n):
    E, K, _, _, _ = batch(oracle, n, 1, SEED + 90 + n, reject=False, canonical=True)
    got, ok = both_placements(eng, E, K)
    D, dok = eng.ris_decompress(E.reshape(n, 32))
    assert dok.all() and ok.all()
    assert got == bytes(eng.ris_compress(eng.msm(D, K.reshape(n, 5)))[0]) == RS.expected(oracle, E, K)[0]


def test_ok_may_be_null_and_an_empty_batch_is_the_empty_sum(eng, oracle):
    E, K, KB, Z, _ = batch(oracle, 300, 2, SEED + 100)
    rc, want, _ = abi(eng, E, K, KB, Z)
    rc2, got, none = abi(eng, E, K, KB, Z, want_ok=False)
    assert (rc, rc2) == (ZC_OK, ZC_OK) and none is None and got == want == RS.expected(oracle, E, K, KB, Z)[0]
    dE, dK, dKB, dZ = (to_dev(x) for x in (E, K, KB, Z))
    out = np.full(32, 0xA5, dtype=np.uint8)
    assert eng.lib.zc_ris_lincomb_sum(eng.ctx, dE.data_ptr(), dK.data_ptr(), 2, dKB.data_ptr(), dZ.data_ptr(), _p(out), None, 300) == ZC_OK
    assert bytes(out) == want
    for kb, z in ((KB, Z), (None, None)):
        rc, got, ok = abi(eng, E[:0], K[:0], None if kb is None else kb[:0], None if z is None else z[:0])
        assert rc == ZC_OK and got == RS.ZERO32 and len(ok) == 0
    out[:] = 0xA5
    assert eng.lib.zc_ris_lincomb_sum(eng.ctx, dE.data_ptr(), dK.data_ptr(), 2, None, None, _p(out), None, 0) == ZC_OK and not out.any()
    got, ok = eng.ris_lincomb_sum(E[:0], K[:0])
    assert got == RS.ZERO32 and ok.shape == (0,)


@pytest.mark.parametrize("backend", ["numpy", "torch"])
def test_framed_buffers(eng, oracle, backend):
    """Rows in the middle of larger allocations, 8 bytes past a 16-byte boundary: no byte outside ok[0..n) and out32 is written,
    no input byte changes, and hostile rows around the inputs do not reach the result."""
    import torch
    n, t = 300, 2
    E, K, KB, Z, _ = batch(oracle, n, t, SEED + 110)
    want, wok = RS.expected(oracle, E, K, KB, Z)
    runs = []
    for fill in (FB.ZERO, FB.HOSTILE):
        out32 = FB.FramedBuffer("output 'out32'", np.full((1, 32), FB.OUT_ROW_FILL, dtype=np.uint8), "numpy", FB.OUT_FRAME_FILL, 8)

        def call(ip, op):
            torch.cuda.synchronize()
            rc = eng.lib.zc_ris_lincomb_sum(eng.ctx, VP(ip[0]), VP(ip[1]), t, VP(ip[2]), VP(ip[3]), VP(out32.ptr), VP(op[0]), n)
            assert rc == ZC_OK, eng.lib.zc_last_error()
            torch.cuda.synchronize()
        inputs = [("in32", E.reshape(n, t * 32), FB.hostile_frame_rows("enc32*%d" % t, oracle)), ("scalars", K.reshape(n, t * 5), FB.hostile_frame_rows("sc*%d" % t)),
                  ("base_scalars", KB, FB.hostile_frame_rows("sc")), ("weights", Z, FB.hostile_frame_rows("sc"))]
        got = FB.run_framed(call, inputs, [("ok", n, 0, np.uint8)], backend=backend, fill=fill, in_shifts=[8] * 4, out_shifts=[8])
        out32.assert_frames_intact()
        runs.append([got[0], out32.rows()])
        assert np.array_equal(got[0], wok) and bytes(out32.rows()[0]) == want
    FB.same_outputs(["ok", "out32"], runs[0], runs[1], "zc_ris_lincomb_sum")


def test_placement_and_argument_errors(eng, oracle):
    lib, ctx = eng.lib, eng.ctx
    n, t = 64, 2
    E, K, KB, Z, _ = batch(oracle, n, t, SEED + 120)
    out, ok = np.full(32, 0xA5, dtype=np.uint8), np.full(n, 0xA5, dtype=np.uint8)
    host = [E.ctypes.data, K.ctypes.data, KB.ctypes.data, Z.ctypes.data, ok.ctypes.data]
    dev_t = [to_dev(x) for x in (E, K, KB, Z, ok)]
    dev = [x.data_ptr() for x in dev_t]
    call = lambda p, o=out.ctypes.data, terms=t, rows=n: lib.zc_ris_lincomb_sum(ctx, p[0], p[1], terms, p[2], p[3], o, p[4], rows)
    for i in range(5):                                                               # one array on the other side
        for a, b in ((host, dev), (dev, host)):
            p = list(a)
            p[i] = b[i]
            assert call(p) == ZC_ERR_MIXED_MEM, i
    dout = to_dev(out)
    assert call(host, dout.data_ptr()) == ZC_ERR_MIXED_MEM and call(dev, dout.data_ptr()) == ZC_ERR_MIXED_MEM
    assert call(host, terms=0) == ZC_ERR_BAD_ARG and call(host, terms=2, rows=1 << 30) == ZC_ERR_BAD_ARG
    assert call(host, rows=(1 << 31) - 1, terms=1) == ZC_ERR_BAD_ARG
    for i in (0, 1):
        p = list(host)
        p[i] = None
        assert call(p) == ZC_ERR_BAD_ARG and lib.zc_last_error().decode().startswith("null pointer: ")
    assert call(host, None) == ZC_ERR_BAD_ARG and lib.zc_last_error() == b"null pointer: out32"
    assert lib.zc_ris_lincomb_sum(None, *host[:2], t, *host[2:4], out.ctypes.data, host[4], n) == ZC_ERR_BAD_ARG
    import torch
    torch.cuda.synchronize()
    assert (out == 0xA5).all() and (ok == 0xA5).all() and bool((dout == 0xA5).all()) and bool((dev_t[4] == 0xA5).all())
    for x, was in zip(dev_t[:4], (E, K, KB, Z)):
        assert np.array_equal(to_host(x), was)
    got, gok = both_placements(eng, E, K, KB, Z)                                     # the context is as usable as before
    assert (got, gok.tolist()) == (lambda r: (r[0], r[1].tolist()))(RS.expected(oracle, E, K, KB, Z))


def test_zc_msm_and_zc_ris_lincomb_are_unchanged_around_it(eng, oracle):
    """The call shares the MSM workspace and the stream: a zc_msm in either regime and a zc_ris_lincomb give the same limbs and
    bytes before and after it, on host arrays and on device tensors."""
    cases = []
    for n in (200, BUCKET_MIN + 1000):
        P = V.base_multiples(oracle, n, SEED + 130 + n)
        cases.append((P, RS.canonical_scalars(n, SEED + 131 + n)))
    E, K, KB, _ = RR.ris_lincomb_rows(oracle, 512, 2, SEED + 132, True)
    snapshot = lambda: ([eng.msm(P, k).copy() for P, k in cases], [eng.msm(to_dev(P), to_dev(k)).copy() for P, k in cases], eng.ris_lincomb(E, K, KB),
                        tuple(to_host(x) for x in eng.ris_lincomb(to_dev(E), to_dev(K), to_dev(KB))))
    before = snapshot()
    assert all(np.array_equal(oracle.ris_compress(m), oracle.ris_compress(oracle.msm_naive_mt(P, k))) for m, (P, k) in zip(before[0], cases))
    RR.assert_same_bytes(before[2], RR.oracle_ris_lincomb(oracle, E, K, KB))
    for n, t in ((100, 2), (BUCKET_MIN + 50, 1), (3, 7)):
        Es, Ks, KBs, Zs, _ = batch(oracle, n, t, SEED + 133 + n)
        got, _ = both_placements(eng, Es, Ks, KBs, Zs)
        assert got == RS.expected(oracle, Es, Ks, KBs, Zs)[0]
        after = snapshot()
        for x, y in zip(before[0] + before[1], after[0] + after[1]):
            assert np.array_equal(x, y)
        RR.assert_same_bytes(after[2], before[2])
        RR.assert_same_bytes(after[3], before[3])
