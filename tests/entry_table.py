"""One description per batched entry point of include/zerocaf_hip.h (this module holds no test).

For every function that takes row buffers the table gives the symbol, the inputs (row width, dtype, what kind of row it is and
a generator), the by-value arguments, the outputs (row width, dtype), the optional mask, where the outputs live, and the
oracle composition that says what the outputs must be -- the one the entry point's own parity test uses.  Several argument
settings of one function are separate entries.  tests/test_entry_table.py keeps the table complete against the header;
tests/test_gpu_buffer_bounds.py runs every entry on framed buffers (tests/framed_buffers.py)."""
import ctypes as C

import numpy as np

from oracle import pymodel as pm
from tests import lincomb_rows as LR
from tests import ris_lincomb_rows as RR
from tests import scalar_ext_rows as SX
from tests import vectors as V

U64, U8 = np.dtype(np.uint64), np.dtype(np.uint8)

# ---- launch thresholds, each beside the rule of dusk_zerocaf_amd/csrc/zc_launch_plan.h it mirrors.  Literals, because this module
# is imported where nothing is compiled; tests/test_launch_plan_emul.py asks the header for the form on both sides of each.
ED_STAGED_MIN_POINTS = 1 << 12          # ED_STAGED_MIN_POINTS (elementwise_form): add / sub / double / neg stage their records ABOVE 2^12 points
QUAD_LAUNCH_ELEMS = 1 << 14             # QUAD_LAUNCH_ELEMS (strict_form): strict scalar-mul batches up to here take four lanes per row
STRICT_SMALL_MAX_ELEMS = 1 << 16        # strict_kernel_for: grid_for(cnt) <= SMALL_LAUNCH_BLOCKS (256 workgroups of ZC_BLOCK = 256 rows) takes the
                                        # independent-chain kernel k_ed_scalar_mul_small, larger batches one workgroup per 256 rows (k_ed_scalar_mul)
PW_MIN_ELEMS = 1 << 17                  # PW_MIN_ELEMS (strict_wants_permutation): strict batches from here on run on persistent waves over the cost-sorted rows
MSM_BUCKET_MIN_N = 4096                 # zc_msm_plan.h MSM_BUCKET_MIN_N: zc_msm shards from here on take the bucket pipeline
MSM_BATCH_BUCKET_MIN_N = 64             # zc_msm_plan.h ZC_MSM_BATCH_BUCKET_MIN_N: zc_msm_batch instances below it are scalar-muls + folds
LINCOMB_MAX_TERMS = 8                   # ZC_LINCOMB_MAX_TERMS (include/zerocaf_hip.h)
WAVE = 64                               # waves of the windowed core own groups of rows: sizes on both sides of one wave

POOL = 331                              # distinct rows per input (a prime above every default size); longer batches repeat them
STD_SIZES = (1, 255, 257, 300)
CORE_SIZES = (WAVE - 1, WAVE + 1, 300)  # the windowed core: FAST, zc_ris_roundtrip_mul, both lincombs
STAGED_POINT_SIZES = (ED_STAGED_MIN_POINTS + 1, ED_STAGED_MIN_POINTS + 301)
STAGED_POINT_ENTRIES = ("zc_ed_add", "zc_ed_sub", "zc_ed_double", "zc_ed_neg")
STAGED_40_ENTRIES = tuple("zc_%s_%s" % (f, op) for f in ("fe", "sc") for op in ("add", "sub", "neg", "mul", "square"))   # ZC_TEST_STREAM_MIN_BYTES
SHARED_INVERSION_ENTRIES = ("zc_fe_invert", "zc_fe_div", "zc_ed_to_affine", "zc_sc_invert")                               # launch_shared_inversions
INV_CHUNKS, INV_SIZES = (2, 7), (300, 301)     # ZC_INV_CHUNK: a ragged last lane (300 = 42 * 7 + 6) and a last lane of one row (301 = 150 * 2 + 1 = 43 * 7)
MSM_BATCH = 3

STRICT, LTR_BIN, BINARY_NAF, FAST = 0, 1, 2, 16
SEED = V.SEED + 0xB0B0


class In:
    """An input: `width` elements of `dtype` per row; kind names the hostile rows its frames can hold
    (framed_buffers.hostile_frame_rows); gen(g) -> (POOL, width) rows; per_n: rows per unit of the call's n."""

    def __init__(self, name, width, dtype, kind, gen, per_n=1):
        self.name, self.width, self.dtype, self.kind, self.gen, self.per_n = name, width, np.dtype(dtype), kind, gen, per_n


class Out:
    """An output: width 0 = one byte per row, flat.  rows: None = the call's n, else that many (the MSM family)."""

    def __init__(self, name, width, dtype, rows=None):
        self.name, self.width, self.dtype, self.rows = name, width, np.dtype(dtype), rows


class Entry:
    """id: the table key (symbol, or symbol + argument setting).  order: the C argument list after ctx, as tokens
    ('in', i) / ('out', j) / ('val', ctypes value) / ('null',) / 'n' / 'id'; the default is inputs, by-value arguments, outputs
    (the mask last), n, trailing arguments.  mask: the index of the optional output, or None.  equal: 'limbs' (bit-identical
    to the oracle) or 'group' (the same group element with the same encodings; the limbs are deterministic).
    place: 'any' (outputs on the device or on the host, like the inputs) or 'host' (outputs in host memory only).
    rowwise: row i of the outputs depends on row i of the inputs only (want is computed once on POOL rows and repeated).
    alias: [(output index, input index)] pairs the header allows to be one buffer.  bases: zc_msm_fixed -- the points of its
    table, which the run creates with zc_msm_bases_create from framed points.  sizes: further batch sizes beside STD_SIZES."""

    def __init__(self, id, ins, outs, want, mid=(), tail=(), mask=None, equal="limbs", place="any", rowwise=True, order=None,
                 alias=(), bases=None, sizes=(), also=()):
        self.id, self.symbol = id, id.split("[")[0]
        self.ins, self.outs, self.want, self.mid, self.tail, self.mask = ins, outs, want, tuple(mid), tuple(tail), mask
        self.equal, self.place, self.rowwise, self.alias, self.bases, self.sizes = equal, place, rowwise, tuple(alias), bases, tuple(sizes)
        self.also = tuple(also)                 # further functions of the header this entry calls on framed buffers (its setup)
        if order is None:
            order = [("in", i) for i in range(len(ins))] + [("val", v) for v in self.mid] + [("out", j) for j in range(len(outs))]
            order += ["n"] + [("val", v) for v in self.tail]
        self.order = order

    def args(self, in_ptrs, out_ptrs, n, table_id=None, null_mask=False):
        a = []
        for tok in self.order:
            if tok == "n":
                a.append(n)
            elif tok == "id":
                a.append(C.c_uint64(table_id))
            elif tok[0] == "in":
                a.append(in_ptrs[tok[1]])
            elif tok[0] == "out":
                a.append(None if null_mask and tok[1] == self.mask else out_ptrs[tok[1]])
            elif tok[0] == "val":
                a.append(tok[1])
            else:
                a.append(None)
        return a

    def out_rows(self, j, n):
        return n if self.outs[j].rows is None else self.outs[j].rows


class Gen:
    """The inputs and the oracle's answers, computed once per process and never changed (arrays are handed out read-only)."""

    def __init__(self, oracle):
        self.oracle = oracle
        self._memo = {}

    def memo(self, key, fn):
        if key not in self._memo:
            v = fn()
            for a in (v if isinstance(v, (list, tuple)) else [v]):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            self._memo[key] = v
        return self._memo[key]

    # ---- pools of POOL rows
    def points(self, salt=0):
        def make():
            k = V.rand_scalars_np(POOL, SEED + 1 + salt, bits=249)
            b = RR.basepoint_rows(POOL)
            P = self.oracle.mt(self.oracle.ed_scalar_mul, b, k)
            P[0 if salt == 0 else 1] = V.IDENT_ROW
            return P
        return self.memo(("points", salt), make)

    def points_q(self):
        def make():
            Q = self.points(1).copy()
            Q[2] = self.points()[2]                                                       # P + P through the unified addition
            Q[3] = self.oracle.ed_neg(self.points()[3:4])[0]                              # P - P
            return Q
        return self.memo("points_q", make)

    def bad_points(self):
        def make():
            P = self.points().copy()
            P[::6, 10:15] = 0                                                             # Z = 0: no affine form, no encoding
            return P
        return self.memo("bad_points", make)

    def fe(self, salt, zeros=0):
        def make():
            a = V.rand_fe_np(POOL, SEED + 10 + salt)
            E = V.limbs_array(V.FE_EDGE if salt % 2 == 0 else list(reversed(V.FE_EDGE)))
            a[:len(E)] = E
            if zeros:
                a[zeros::7] = 0
            return a
        return self.memo(("fe", salt, zeros), make)

    def sc(self, salt):
        """canonical scalars (below L) with the edge set"""
        def make():
            a = V.rand_fe_np(POOL, SEED + 30 + salt, pm.L)
            E = V.limbs_array(V.SC_EDGE if salt % 2 == 0 else list(reversed(V.SC_EDGE)))
            a[:len(E)] = E
            return a
        return self.memo(("sc", salt), make)

    def raw_sc(self, salt, bits=252, edges=True):
        """Mul<Scalar> operands: raw limbs, zero, one, L, all ones and the patterns at or above 2^256"""
        def make():
            K = V.rand_scalars_np(POOL, SEED + 50 + salt, bits=bits)
            if edges:
                head = np.array([[0] * 5, [1, 0, 0, 0, 0], pm.limbs(pm.L), pm.limbs(2**249 - 1), [(1 << 52) - 1] * 5, pm.limbs(pm.L - 1)], dtype=np.uint64)
                K[:len(head)] = head
                raw = V.raw_scalar_edges(n_random=8)
                K[8:8 + len(raw)] = raw
            return K
        return self.memo(("raw_sc", salt, bits, edges), make)

    def invertible_sc(self):
        def make():
            a = SX.random_invert_rows(POOL, SEED + 70)
            zeros = np.array([w for _, w in SX.zero_patterns()], dtype=np.uint64)
            a[5:5 + 7 * len(zeros):7] = zeros
            a[POOL - 1] = 0
            a[299], a[300] = zeros[1], zeros[2]                                           # the ragged ends of the chunked forms
            return a
        return self.memo("invertible_sc", make)

    def bytes(self, salt, width=32):
        return self.memo(("bytes", salt, width), lambda: np.random.default_rng(SEED + 90 + salt).integers(0, 256, size=(POOL, width), dtype=np.uint8))

    def sc_bytes(self):
        def make():
            b = self.bytes(1).copy()
            b[::2, 31] = 0                                                                # below L; nearly all others are refused
            return b
        return self.memo("sc_bytes", make)

    def ris_enc(self):
        def make():
            e = self.oracle.ris_compress(self.points()).copy()
            e[::4] = self.bytes(2)[::4]
            return e
        return self.memo("ris_enc", make)

    def ed_enc(self):
        def make():
            e = self.oracle.ed_compress(self.points())[0].copy()
            e[::3] = self.bytes(3)[::3]
            return e
        return self.memo("ed_enc", make)

    def lincomb(self, t):
        """(P (POOL, t * 20), K (POOL, t * 5)) of tests/lincomb_rows.py, planted rows included"""
        def make():
            pool = np.concatenate([self.points(), self.points_q()])
            pts = lambda count, s: pool[(np.arange(count) * 7 + s) % len(pool)]
            P, K, _ = LR.lincomb_rows(self.oracle, LINCOMB_GEN_ROWS, t, SEED + 100 + t, points=pts)
            sel = _planted_first()
            return np.ascontiguousarray(P[sel].reshape(POOL, t * 20)), np.ascontiguousarray(K[sel].reshape(POOL, t * 5))
        return self.memo(("lincomb", t), make)

    def ris_lincomb(self, t, base):
        def make():
            pool = np.concatenate([self.points(), self.points_q()])
            pts = lambda count, s: pool[(np.arange(count) * 7 + s) % len(pool)]
            E, K, KB, _ = RR.ris_lincomb_rows(self.oracle, LINCOMB_GEN_ROWS, t, SEED + 120 + t, base, points=pts)
            sel = _planted_first()
            return (np.ascontiguousarray(E[sel].reshape(POOL, t * 32)), np.ascontiguousarray(K[sel].reshape(POOL, t * 5)),
                    None if KB is None else np.ascontiguousarray(KB[sel]))
        return self.memo(("ris_lincomb", t, base), make)


LINCOMB_GEN_ROWS = 479                  # tests/lincomb_rows.py plants its 68 row families at rows 3, 10, ... 472, ris_lincomb_rows at 5, 12, ...


def _planted_first():
    """POOL of the LINCOMB_GEN_ROWS generated rows: those that hold planted families first, so that every size sees some."""
    planted = [i for i in range(LINCOMB_GEN_ROWS) if i % 7 in (2, 3, 5)]          # (2: the planted base scalars)
    return np.array(planted + [i for i in range(LINCOMB_GEN_ROWS) if i % 7 not in (2, 3, 5)])[:POOL]


def rows_of(pool, n):
    """n rows: the pool repeated"""
    pool = np.asarray(pool)
    return np.ascontiguousarray(np.concatenate([pool] * (n // len(pool) + 1))[:n]) if n > len(pool) else np.ascontiguousarray(pool[:n])


def aslist(x):
    return list(x) if isinstance(x, (tuple, list)) else [x]


def ora(name, *extra):
    """want = the oracle function `name` over the inputs (on all host cores)"""
    return lambda g, *a: aslist(g.oracle.mt(getattr(g.oracle, name), *a, extra=extra))


# ---------------------------------------------------------------- inputs
FE_A = In("a", 5, U64, "fe", lambda g: g.fe(0))
FE_B = In("b", 5, U64, "fe", lambda g: g.fe(1))
FE_A0 = In("a", 5, U64, "fe", lambda g: g.fe(2, zeros=1))         # rows that are not invertible
FE_B0 = In("b", 5, U64, "fe", lambda g: g.fe(3, zeros=3))
FE_E = In("e", 5, U64, "fe", lambda g: g.fe(4))
SC_A = In("a", 5, U64, "sc", lambda g: g.sc(0))
SC_B = In("b", 5, U64, "sc", lambda g: g.sc(1))
SC_C = In("c", 5, U64, "sc", lambda g: g.sc(2))
SC_RAW = In("a", 5, U64, "sc", lambda g: g.raw_sc(0, bits=260, edges=False))
SC_INV = In("a", 5, U64, "sc", lambda g: g.invertible_sc())
K_RAW = In("k", 5, U64, "sc", lambda g: g.raw_sc(1))
K_CANON = In("k", 5, U64, "sc", lambda g: g.raw_sc(2, bits=248, edges=False))
PT_P = In("p", 20, U64, "pt", lambda g: g.points())
PT_Q = In("q", 20, U64, "pt", lambda g: g.points_q())
PT_BAD = In("p", 20, U64, "pt", lambda g: g.bad_points())
PJ_P = In("p", 15, U64, "proj", lambda g: np.ascontiguousarray(g.points()[:, :15]))
PJ_BAD = In("p", 15, U64, "proj", lambda g: np.ascontiguousarray(g.bad_points()[:, :15]))          # Z = 0 among them
PJ_Q = In("q", 15, U64, "proj", lambda g: np.ascontiguousarray(g.points_q()[:, :15]))
ENC_RIS = In("in32", 32, U8, "enc32", lambda g: g.ris_enc())
ENC_ED = In("in32", 32, U8, "enc32", lambda g: g.ed_enc())
BYTES32 = In("in32", 32, U8, "enc32", lambda g: g.bytes(0))
SC_BYTES = In("in32", 32, U8, "scbytes", lambda g: g.sc_bytes())
BYTES64 = In("in64", 64, U8, "bytes64", lambda g: g.bytes(4, 64))

O5, O10, O15, O20, O80 = Out("out", 5, U64), Out("xy_out", 10, U64), Out("out", 15, U64), Out("out", 20, U64), Out("out4", 80, U64)
O32, FLAG, OK, BITS = Out("out32", 32, U8), Out("flag", 0, U8), Out("ok", 0, U8), Out("bits256", 256, U8)
ONE_POINT = Out("out_point", 20, U64, rows=1)
BATCH_POINTS = Out("out_points", 20, U64, rows=MSM_BATCH)

ENTRIES = []


def add(*a, **kw):
    ENTRIES.append(Entry(*a, **kw))


# ---------------------------------------------------------------- FieldElement
for _op in ("add", "sub", "mul", "pow"):
    add("zc_fe_" + _op, [FE_A, FE_E if _op == "pow" else FE_B], [O5], ora("fe_" + _op))
for _op in ("neg", "square", "half"):
    add("zc_fe_" + _op, [FE_A], [O5], ora("fe_" + _op))
add("zc_fe_invert", [FE_A0], [O5, OK], ora("fe_invert"), mask=1, alias=[(0, 0)])
add("zc_fe_div", [FE_A0, FE_B0], [O5, OK], ora("fe_div"), mask=1, alias=[(0, 0), (0, 1)])
add("zc_fe_legendre_symbol", [FE_A], [FLAG], ora("fe_legendre_symbol"))
add("zc_fe_is_positive", [FE_A], [FLAG], ora("fe_is_positive"))
for _s in (0, 1):
    add("zc_fe_mod_sqrt[sign=%d]" % _s, [FE_A], [O5, OK], ora("fe_mod_sqrt", _s), mid=(C.c_int(_s),), mask=1)
add("zc_fe_from_bytes", [BYTES32], [O5], ora("fe_from_bytes"))
add("zc_fe_to_bytes", [FE_A], [O32], ora("fe_to_bytes"))
add("zc_fe_sqrt_ratio_i", [FE_A0, FE_B0], [O5, Out("was_square", 0, U8)], ora("fe_sqrt_ratio_i"), mask=1)
add("zc_fe_inv_sqrt", [FE_A0], [O5, Out("was_square", 0, U8)], ora("fe_inv_sqrt"), mask=1)

# ---------------------------------------------------------------- Scalar
for _op in ("add", "sub", "mul", "pow"):
    add("zc_sc_" + _op, [SC_A, SC_B], [O5], ora("sc_" + _op))
for _op in ("neg", "square", "half"):
    add("zc_sc_" + _op, [SC_A], [O5], ora("sc_" + _op))
add("zc_sc_from_bytes", [SC_BYTES], [O5, OK], ora("sc_from_bytes"), mask=1)
add("zc_sc_to_bytes", [SC_A], [O32], ora("sc_to_bytes"))
for _sh in (0, 1, 255):
    add("zc_sc_shr[shift=%d]" % _sh, [SC_RAW], [O5], ora("sc_shr", _sh), mid=(C.c_uint(_sh),))
add("zc_sc_into_bits", [SC_RAW], [BITS], ora("sc_into_bits"))
for _w in (0, 2, 7):
    add("zc_sc_compute_naf[width=%d]" % _w, [SC_RAW], [Out("naf256", 256, U8)],
        (lambda w: lambda g, a: [g.oracle.mt(g.oracle.sc_compute_naf, a, extra=(w,)).view(np.uint8)])(_w), mid=(C.c_uint(_w),))


def _le_values(b):
    return [int.from_bytes(bytes(r), "little") for r in b]


add("zc_sc_from_bytes_wide", [BYTES64], [O5], lambda g, b: [SX.canon_rows(_le_values(b))])
add("zc_sc_from_bytes_mod_order", [BYTES32], [O5], lambda g, b: [SX.canon_rows(_le_values(b))])
add("zc_sc_muladd", [SC_RAW, SC_B, SC_C], [O5], lambda g, a, b, c: [SX.muladd_expected(a, b, c)])
add("zc_sc_invert", [SC_INV], [O5, OK], lambda g, a: list(SX.invert_expected(a)), mask=1, alias=[(0, 0)])

# ---------------------------------------------------------------- EdwardsPoint
add("zc_ed_add", [PT_P, PT_Q], [O20], ora("ed_add"))
add("zc_ed_sub", [PT_P, PT_Q], [O20], ora("ed_sub"))
add("zc_ed_double", [PT_P], [O20], ora("ed_double"))
add("zc_ed_neg", [PT_P], [O20], ora("ed_neg"))
add("zc_ed_scalar_mul[STRICT]", [PT_P, K_RAW], [O20], ora("ed_scalar_mul"), tail=(C.c_uint(STRICT),))
add("zc_ed_scalar_mul[LTR_BIN]", [PT_P, K_CANON], [O20], ora("ed_scalar_mul_mode", LTR_BIN), tail=(C.c_uint(LTR_BIN),))
add("zc_ed_scalar_mul[BINARY_NAF]", [PT_P, K_CANON], [O20], ora("ed_scalar_mul_mode", BINARY_NAF), tail=(C.c_uint(BINARY_NAF),))
add("zc_ed_scalar_mul[FAST]", [PT_P, K_RAW], [O20], ora("ed_scalar_mul"), tail=(C.c_uint(FAST),), equal="group", sizes=CORE_SIZES)
for _k in (0, 1, 249):
    add("zc_ed_mul_by_pow_2[kexp=%d]" % _k, [PT_P], [O20], ora("ed_mul_by_pow_2", _k), mid=(C.c_uint64(_k),))
add("zc_ed_mul_by_cofactor", [PT_P], [O20], ora("ed_mul_by_pow_2", 3))
add("zc_ed_to_affine", [PT_BAD], [O10, OK], ora("ed_to_affine"), mask=1)
add("zc_ed_eq", [PT_P, PT_Q], [FLAG], ora("ed_eq"))
add("zc_ed_compress", [PT_BAD], [O32, OK], ora("ed_compress"), mask=1)
add("zc_ed_decompress", [ENC_ED], [O20, OK], ora("ed_decompress"), mask=1)
add("zc_ed_is_valid", [PT_BAD], [FLAG], ora("ed_is_valid"))
add("zc_ed_coset4", [PT_P], [O80], ora("ed_coset4"))

# ---------------------------------------------------------------- Ristretto
add("zc_ris_compress", [PT_P], [O32], ora("ris_compress"))
add("zc_ris_decompress", [ENC_RIS], [O20, OK], ora("ris_decompress"), mask=1)
add("zc_ris_eq", [PT_P, PT_Q], [FLAG], ora("ris_eq"))
add("zc_ris_roundtrip_mul", [ENC_RIS, K_RAW], [O32, OK], ora("ris_roundtrip_mul"), mask=1, sizes=CORE_SIZES)
add("zc_ris_is_valid", [PT_P], [FLAG], ora("ris_is_valid"))
add("zc_ris_elligator", [FE_A], [O20], ora("ris_elligator"))
add("zc_ris_from_uniform_bytes", [BYTES64], [O20], ora("ris_from_uniform_bytes"))

# ---------------------------------------------------------------- ProjectivePoint
add("zc_proj_add", [PJ_P, PJ_Q], [O15], ora("proj_add"))
add("zc_proj_sub", [PJ_P, PJ_Q], [O15], ora("proj_sub"))
add("zc_proj_double", [PJ_P], [O15], ora("proj_double"))
add("zc_proj_neg", [PJ_P], [O15], ora("proj_neg"))
add("zc_proj_to_extended", [PJ_P], [O20], ora("proj_to_extended"))


def _proj_eq(g, p, q):
    eq, ok = g.oracle.proj_eq(p, q)
    return [eq & ok]                                                                      # Z = 0 compares unequal


add("zc_proj_eq", [PJ_BAD, PJ_Q], [FLAG], _proj_eq)
add("zc_proj_is_valid", [PJ_P], [FLAG], ora("proj_is_valid"))
add("zc_proj_scalar_mul", [PJ_Q, K_RAW], [O15], ora("proj_scalar_mul"))


# ---------------------------------------------------------------- fixed base
def _k_times_base(g, k):
    return g.oracle.mt(g.oracle.ed_scalar_mul, RR.basepoint_rows(len(k)), k)


add("zc_ed_mul_base", [K_RAW], [O20], lambda g, k: [_k_times_base(g, k)], equal="group")
add("zc_ris_mul_base_compress", [K_RAW], [O32], lambda g, k: [g.oracle.ris_compress(_k_times_base(g, k))])
def _wnaf_times_base(width):
    """(sum_i d_i 2^i) B for the digits d of the reference's compute_window_NAF(width): what the header promises and
    tests/test_gpu_parity.py checks -- k B itself except near L, where the reference's digits stand for another integer."""
    def want(g, k):
        naf = np.asarray(g.oracle.sc_compute_naf(k, width)).astype(np.int64)
        return [_k_times_base(g, V.limbs_array([sum(int(d) << i for i, d in enumerate(row)) % pm.L for row in naf]))]
    return want


K_WNAF = In("k", 5, U64, "sc", lambda g: g.sc(3))
for _w in (2, 7):
    add("zc_ed_mul_base_wnaf[width=%d]" % _w, [K_WNAF], [O20], _wnaf_times_base(_w), mid=(C.c_uint(_w),), equal="group")

# ---------------------------------------------------------------- linear combinations per row
for _t in (1, 3, LINCOMB_MAX_TERMS):
    add("zc_ed_lincomb[terms=%d]" % _t,
        [In("points", 20 * _t, U64, "pt*%d" % _t, (lambda t: lambda g: g.lincomb(t)[0])(_t)),
         In("scalars", 5 * _t, U64, "sc*%d" % _t, (lambda t: lambda g: g.lincomb(t)[1])(_t))],
        [O20], (lambda t: lambda g, P, K: [LR.oracle_lincomb(g.oracle, P.reshape(-1, t, 20), K.reshape(-1, t, 5))])(_t),
        mid=(C.c_size_t(_t),), equal="group", sizes=CORE_SIZES)
for _t, _base in ((1, False), (LINCOMB_MAX_TERMS, False), (1, True), (LINCOMB_MAX_TERMS - 1, True)):
    _ins = [In("in32", 32 * _t, U8, "enc32*%d" % _t, (lambda t, b: lambda g: g.ris_lincomb(t, b)[0])(_t, _base)),
            In("scalars", 5 * _t, U64, "sc*%d" % _t, (lambda t, b: lambda g: g.ris_lincomb(t, b)[1])(_t, _base))]
    if _base:
        _ins.append(In("base_scalars", 5, U64, "sc", (lambda t, b: lambda g: g.ris_lincomb(t, b)[2])(_t, _base)))
    add("zc_ris_lincomb[terms=%d%s]" % (_t, ",base" if _base else ""), _ins, [O32, OK],
        (lambda t: lambda g, E, K, KB=None: list(RR.oracle_ris_lincomb(g.oracle, E.reshape(-1, t, 32), K.reshape(-1, t, 5), KB)))(_t),
        mask=1, sizes=CORE_SIZES,
        order=[("in", 0), ("in", 1), ("val", C.c_size_t(_t)), ("in", 2) if _base else ("null",), ("out", 0), ("out", 1), "n"])


# ---------------------------------------------------------------- MSM family: one sum per instance, not one output per row
def _msm_want(g, P, K):
    return [g.oracle.msm_naive_mt(P, K)]


def _msm_batch_want(g, P, K):
    n = len(P) // MSM_BATCH
    return [np.concatenate([g.oracle.msm_naive_mt(P[b * n:(b + 1) * n], K[b * n:(b + 1) * n]) for b in range(MSM_BATCH)])]


def _fold_want(g, parts):
    acc = parts[0:1]
    for i in range(1, len(parts)):
        acc = g.oracle.ed_add(acc, parts[i:i + 1])
    return [np.ascontiguousarray(acc)]


MSM_SIZES = (MSM_BUCKET_MIN_N,)                    # the smallest shard that takes the bucket pipeline
K_MSM = In("scalars", 5, U64, "sc", lambda g: g.raw_sc(1))
K_MSM3 = In("scalars", 5, U64, "sc", lambda g: g.raw_sc(1), per_n=MSM_BATCH)
PT_MSM3 = In("points", 20, U64, "pt", lambda g: g.points(), per_n=MSM_BATCH)
add("zc_msm", [PT_P, K_MSM], [ONE_POINT], _msm_want, equal="group", place="host", rowwise=False, sizes=MSM_SIZES,
    order=[("in", 0), ("in", 1), "n", ("out", 0)])
add("zc_msm_partial", [PT_P, K_MSM], [Out("out_dev_point", 20, U64, rows=1)], _msm_want, equal="group", place="device", rowwise=False, sizes=MSM_SIZES,
    order=[("in", 0), ("in", 1), "n", ("out", 0)])
add("zc_ed_fold_ordered", [PT_P], [Out("out", 20, U64, rows=1)], _fold_want, rowwise=False, order=[("in", 0), "n", ("out", 0)])
add("zc_msm_fixed", [K_MSM3], [BATCH_POINTS], lambda g, K, bases=None: _msm_batch_want(g, np.concatenate([bases] * MSM_BATCH), K),
    equal="group", place="host", rowwise=False, sizes=MSM_SIZES, bases=PT_P, also=("zc_msm_bases_create",), order=["id", ("in", 0), ("val", C.c_size_t(MSM_BATCH)), ("out", 0)])
add("zc_msm_batch", [PT_MSM3, K_MSM3], [BATCH_POINTS], _msm_batch_want, equal="group", place="host", rowwise=False,
    sizes=(MSM_BATCH_BUCKET_MIN_N - 1,) + MSM_SIZES, order=[("in", 0), ("in", 1), "n", ("val", C.c_size_t(MSM_BATCH)), ("out", 0)])

TABLE = {e.id: e for e in ENTRIES}
assert len(TABLE) == len(ENTRIES)

# ---------------------------------------------------------------- functions of the header that take no row buffers
EXCLUDED = {
    "zc_ctx_create": "context: creates the context, takes a list of device numbers",
    "zc_ctx_destroy": "context: takes no buffers",
    "zc_ctx_device": "context query",
    "zc_ctx_device_count": "context query",
    "zc_ctx_set_stream": "stream binding",
    "zc_ctx_set_stream_dev": "stream binding",
    "zc_ctx_synchronize": "stream wait",
    "zc_device_count": "query without buffers",
    "zc_last_error": "query without buffers",
    "zc_version": "query without buffers",
    "zc_host_register": "pins the caller's buffer; neither reads nor writes its rows",
    "zc_host_unregister": "the counterpart of zc_host_register",
    "zc_msm_plan": "plan query: no device work; its output is an int32 list bounded by nout (tests/test_gpu_parity.py)",
    "zc_msm_fixed_plan": "plan query",
    "zc_msm_batch_plan": "plan query",
    "zc_msm_bases_destroy": "frees a table by id",
    "zc_comm_unique_id": "communicator",
    "zc_comm_init": "communicator",
    "zc_comm_destroy": "communicator",
    "zc_comm_size": "communicator query",
    "zc_msm_sharded": "needs a communicator of several ranks (tests/test_multi_gpu_rccl.py)",
}


def prototypes(header_text):
    """[(name, argument list text)] of the functions a C header declares, comments stripped."""
    import re
    text = re.sub(r"/\*.*?\*/", "", header_text, flags=re.S)
    return [(m.group(1), " ".join(m.group(2).split())) for m in re.finditer(r"\b(zc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)]


def coverage_gaps(header_text, table=None, excluded=None):
    """(functions of the header that are neither in the table nor excluded, names of the table or the exclusions that the
    header does not declare, names that are both in the table and excluded)"""
    table = TABLE if table is None else table
    excluded = EXCLUDED if excluded is None else excluded
    declared = [name for name, _ in prototypes(header_text)]
    covered = {s for e in table.values() for s in (e.symbol,) + e.also}
    missing = [f for f in declared if f not in covered and f not in excluded]
    unknown = sorted((covered | set(excluded)) - set(declared))
    return missing, unknown, sorted(covered & set(excluded))
