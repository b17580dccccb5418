"""Rows and the model for the tests of the point sums (zc_ed_sum_rows, zc_ris_sum_rows: CPU emulation and GPU tier).

parts(terms) restates the order of association of include/zerocaf_hip_ext_sum_rows.h in Python, independently of the C plan
(tests/test_sum_rows_plan_emul.py compares the two); model_sum applies the oracle's ed_add in exactly that order, one batched
call per fold step and per tree level.  Points come from the classes of tests/point_classes.py (subgroup, torsion, mixed
order, decoded, scaled, the identity); row i of a batch depends on i and `terms` only, so a batch of n rows is a prefix of
every longer one.  By i mod 8: 1 one point repeated, 2 P followed by -P, 7 all identity, 5 identities sprinkled in, otherwise a
walk through the pool.  The wire rows are encodings of doubled pool points (always decodable) and the zero encoding; rows with
i mod 8 in (1, 3, 6) carry an undecodable encoding in the first, a middle and the last term position."""
import ctypes as C

import numpy as np

from tests import hostile_rows as HR
from tests import point_classes as PC
from tests import vectors as V

SEED = V.SEED + 0x5352
M52 = (1 << 52) - 1
SERIAL_MAX, MIN_SLICE, MAX_PARTS, BLOCK = 32, 16, 1 << 16, 256      # restated from the header's text, not read from the C plan
SHORT_TERMS = [0, 1, 2, 3, 8, 31, 32, 33, 47]                       # 32 | 33: the serial limit and the first count with 2 parts; 47: uneven slices (24 + 23)
LONG_TERMS = [4095, 4096, 8191, 8192, 8197]                         # 128 | 256 parts; 256 | 512 parts (one kernel | two); 8197: uneven, two kernels
SHORT_N = [1, 63, 65, 257, 1000]
LONG_N = [1, 3]

_cache = {}


def parts(terms):
    """P of the header: 1 up to 32 terms; otherwise the largest power of two with 16 P <= terms, at most 2^16."""
    if terms <= SERIAL_MAX:
        return 1
    p = 1
    while 2 * p <= MAX_PARTS and MIN_SLICE * 2 * p <= terms:
        p *= 2
    return p


def model_sum(oracle, pts):
    """(n, terms, 20) -> (n, 20): slices s, s + P, ... folded from the left, then adjacent pairs level by level; every step one
    batched oracle.ed_add."""
    pts = np.ascontiguousarray(pts, dtype=np.uint64)
    n, terms = pts.shape[:2]
    if terms == 0 or n == 0:
        return PC.ident_rows(n).reshape(n, 20)
    P = parts(terms)
    add = lambda a, b: oracle.mt(oracle.ed_add, np.ascontiguousarray(a.reshape(-1, 20)), np.ascontiguousarray(b.reshape(-1, 20))).reshape(a.shape)
    acc = pts[:, :P].copy()
    k = 1
    while k * P < terms:
        cnt = min(P, terms - k * P)
        acc[:, :cnt] = add(acc[:, :cnt], pts[:, k * P:k * P + cnt])
        k += 1
    while acc.shape[1] > 1:
        acc = add(acc[:, 0::2], acc[:, 1::2])
    return np.ascontiguousarray(acc[:, 0])


def pool(oracle):
    """(57, 20) canonical valid points: eight of every class of point_classes and the identity, read-only."""
    if "pool" not in _cache:
        cl = PC.classes(oracle, 8, SEED)
        rows = np.concatenate([cl[name] for name in ("subgroup", "torsion", "order_2L", "order_4L", "order_8L", "decoded", "scaled")] + [PC.ident_rows(1)])
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        assert rows.shape == (57, 20) and (rows <= M52).all()
        rows.setflags(write=False)
        _cache["pool"] = rows
        neg = oracle.ed_neg(rows)
        neg.setflags(write=False)
        _cache["neg"] = neg
    return _cache["pool"]


def _index(n, terms):
    i, j = np.arange(n)[:, None], np.arange(terms)[None, :]
    return (5 * i + 11 * j + (i // 8) * (j // 3)) % 56             # never the identity (pool row 56) by itself


def points(oracle, n, terms):
    """(n, terms, 20), read-only and cached per terms at the largest n asked for so far (rows are prefixes of one another)."""
    key = ("pts", terms)
    if key not in _cache or len(_cache[key]) < n:
        pl = pool(oracle)
        neg = _cache["neg"]
        idx = _index(n, terms)
        out = pl[idx]
        kind = np.arange(n) % 8
        if terms:
            r = kind == 1
            out[r] = pl[idx[r, :1]]                                 # one point, repeated
            r = np.flatnonzero(kind == 2)
            for j in range(1, terms, 2):
                out[r, j] = neg[idx[r, j - 1]]                      # P followed by -P
            out[kind == 7] = pl[56]                                 # all identity
            r = kind == 5
            out[r, ::3] = pl[56]                                    # identities among the terms
        out = np.ascontiguousarray(out)
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key][:n]


def want_ed(oracle, n, terms):
    key = ("want", terms)
    if key not in _cache or len(_cache[key]) < n:
        w = model_sum(oracle, points(oracle, n, terms))
        w.setflags(write=False)
        _cache[key] = w
    return _cache[key][:n]


def undecodable(oracle):
    return [b for _, b in HR.undecodable(oracle.ris_decompress)]


def FBROWS(oracle):
    """the hostile 32-byte rows of tests/framed_buffers.py"""
    from tests import framed_buffers as FB
    return FB.hostile_frame_rows("enc32", oracle)


def bad_position(i, terms):
    """The term position of row i's undecodable encoding, or None."""
    if terms == 0:
        return None
    return {1: 0, 3: terms // 2, 6: terms - 1}.get(i % 8)


def encodings(oracle, n, terms):
    """((n, terms, 32) uint8, (n,) expected accept bits)."""
    key = ("enc", terms)
    if key not in _cache or len(_cache[key][0]) < n:
        pl = pool(oracle)
        table = oracle.ris_compress(oracle.ed_double(pl))           # 2 P is in the even subgroup: its encoding decodes
        assert oracle.ris_decompress(table)[1].all() and not table[56].any()
        idx = _index(n, terms)
        idx[np.arange(n) % 8 == 7] = 56
        enc = table[idx]
        ok = np.ones(n, dtype=np.uint8)
        bad = undecodable(oracle)
        for i in range(n):
            j = bad_position(i, terms)
            if j is not None:
                enc[i, j] = bad[(i // 8) % len(bad)]
                ok[i] = 0
        enc = np.ascontiguousarray(enc)
        enc.setflags(write=False)
        ok.setflags(write=False)
        _cache[key] = (enc, ok)
    enc, ok = _cache[key]
    return enc[:n], ok[:n]


def want_wire(oracle, n, terms):
    """((n, 32) bytes, (n,) ok): the oracle's decompress of every term, its additions, its ris_compress; refused rows zeroed."""
    key = ("wwire", terms)
    if key not in _cache or len(_cache[key][0]) < n:
        enc, ok = encodings(oracle, n, terms)
        pts, dec = oracle.mt(oracle.ris_decompress, np.ascontiguousarray(enc.reshape(-1, 32))) if terms else (np.zeros((0, 20), dtype=np.uint64), np.zeros(0, dtype=np.uint8))
        assert np.array_equal(dec.reshape(n, terms).all(axis=1), ok == 1)
        out = oracle.mt(oracle.ris_compress, model_sum(oracle, pts.reshape(n, terms, 20)))
        out[ok == 0] = 0
        out.setflags(write=False)
        _cache[key] = (out, ok)
    out, ok = _cache[key]
    return out[:n], ok[:n]


# ------------------------------------------------------------------ the host-emulation library (tests/emul/sum_rows_emul.cpp)
def _p(a):
    return C.c_void_p(a.ctypes.data)


class Emul:
    """One build of tests/emul/sum_rows_emul.cpp.  Outputs are framed by one row on either side; inputs are compared afterwards."""

    def __init__(self, lib):
        self.lib = lib
        lib.emul_sum_parts.restype = C.c_size_t
        lib.emul_sum_parts.argtypes = [C.c_size_t]

    def parts(self, terms):
        return self.lib.emul_sum_parts(terms)

    def plan(self, n, terms):
        out = np.zeros(9, dtype=np.uint64)
        self.lib.emul_sum_plan(C.c_size_t(n), C.c_size_t(terms), _p(out))
        return dict(zip(("parts", "steps", "form", "rows_per_block", "blocks_per_row", "grid1", "grid2", "partials", "workspace_bytes"), (int(x) for x in out)))

    def constants(self):
        out = np.zeros(6, dtype=np.uint64)
        self.lib.emul_sum_constants(_p(out))
        return dict(zip(("serial_max", "min_slice", "max_parts", "block", "partial_words", "index_limit"), (int(x) for x in out)))

    def fold_steps(self, terms, parts):
        self.lib.emul_sum_fold_steps.restype = C.c_uint32
        return self.lib.emul_sum_fold_steps(C.c_uint32(terms), C.c_uint32(parts))

    def decode_differs(self, enc):
        """encodings on which the fold's decoder and ris_decompress disagree in verdict or in a limb of the point"""
        enc = np.ascontiguousarray(enc, dtype=np.uint8).reshape(-1, 32)
        self.lib.emul_decode_differs.restype = C.c_size_t
        return self.lib.emul_decode_differs(_p(enc), C.c_size_t(len(enc)))

    def too_large(self, n, terms):
        return self.lib.emul_sum_too_large(C.c_size_t(n), C.c_size_t(terms)) == 1

    def _framed(self, n, width, dtype):
        buf = np.full(width * (n + 2), 0xA5, dtype=dtype)
        return buf, buf[width:width * (n + 1)]

    def ed(self, pts):
        pts = np.ascontiguousarray(pts, dtype=np.uint64)
        n, terms = pts.shape[:2]
        before = pts.copy()
        buf, out = self._framed(n, 20, np.uint64)
        self.lib.emul_ed_sum_rows(_p(pts), C.c_size_t(terms), _p(out), C.c_size_t(n))
        assert (buf[:20] == 0xA5).all() and (buf[20 * (n + 1):] == 0xA5).all() and np.array_equal(pts, before)
        return out.reshape(n, 20).copy()

    def wire(self, enc, with_ok=True):
        enc = np.ascontiguousarray(enc, dtype=np.uint8)
        n, terms = enc.shape[:2]
        before = enc.copy()
        buf, out = self._framed(n, 32, np.uint8)
        okbuf, ok = self._framed(n, 1, np.uint8)
        self.lib.emul_ris_sum_rows(_p(enc), C.c_size_t(terms), _p(out), _p(ok) if with_ok else None, C.c_size_t(n))
        assert (buf[:32] == 0xA5).all() and (buf[32 * (n + 1):] == 0xA5).all() and okbuf[0] == 0xA5 and okbuf[-1] == 0xA5 and np.array_equal(enc, before)
        return out.reshape(n, 32).copy(), ok.copy()


MUTANT_TERMS = [0, 1, 2, 3, 8, 33, 47, 100, 4096, 8197]             # 100: 4 parts, the first tree with an odd s


def failures(lib, oracle, terms_list=MUTANT_TERMS):
    """The checks of the emulation tier on one build, as labels of those that failed, per term count: "ed" (limbs against
    model_sum), "ed_eq" (the same group element and the same compressed bytes, whatever the limbs) and "wire" (bytes and accept
    bits); 9 rows for the short counts, 2 for the long ones."""
    em, failed = Emul(lib), []
    for terms in terms_list:
        n = 2 if terms > 1000 else 9
        got, want = em.ed(points(oracle, n, terms)), np.ascontiguousarray(want_ed(oracle, n, terms))
        if not np.array_equal(got, want):
            failed.append("ed [terms=%d]" % terms)
        if not (oracle.ed_eq(got, want).all() and np.array_equal(oracle.ris_compress(got), oracle.ris_compress(want))):
            failed.append("ed_eq [terms=%d]" % terms)
        wb, wok = want_wire(oracle, n, terms)
        out, ok = em.wire(encodings(oracle, n, terms)[0])
        if not (np.array_equal(out, wb) and np.array_equal(ok, wok)):
            failed.append("wire [terms=%d]" % terms)
    return failed
