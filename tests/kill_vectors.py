"""Kill vectors: named families of inputs chosen for the lines of zc_arith.hip.h / zc_curve.hip.h that seeded uniform values
do not reach -- sign boundaries, degenerate encodings, zeros by value, the longest inversions found, recoding carries --
next to compact families for the plain arithmetic and group law.  tests/mutants.py names, per planted defect, the family
that must catch it; tests/test_mutants_emul.py plants the defects in temporary host builds; tests/test_gpu_kill_vectors.py
sends the same rows through the C ABI.

A family is a list of `Case`s built once: an abstract operation, input rows, expected output rows.  Expected values are
Python integers (oracle/pymodel.py) except the two left-to-right scalar multiplications, whose limbs come from the C oracle.
`run(family, backend)` returns the comparisons that failed.  A backend answers `call(case)` with the outputs, or None where
it has no such operation: `EmulBackend` wraps one host-emulation library (tests/emul/*.cpp), `EngineBackend` an Engine.

Operations with several launch forms: `Form` names one, `EngineBackend(form=...)` runs only the cases that have it, and
`packed` reorders a `mulmod` case so that whole waves take one product form (tests/test_kill_vector_waves.py holds the wave
model, tests/test_gpu_kill_vector_forms.py the forms).  `Case.bad_rows` names the rows behind a failed comparison.
"""
import ctypes as C
import importlib.util
import json
import os
import random

import numpy as np

from oracle import pymodel as pm
from tests import scalar_ext_rows as S
from tests import vectors as V

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
P, L = pm.P, pm.L
HALF = (P - 1) // 2
SEED = V.SEED + 0x4B11
M52 = (1 << 52) - 1
INV_CHUNKS = (2, 7, 64)

# family -> the emulation source its operations live in
LIBS = {"arith": "emul.cpp", "scalar_ext": "scalar_ext_emul.cpp", "lincomb": "lincomb_emul.cpp", "ris_lincomb": "ris_lincomb_emul.cpp",
        "sm_tile": "sm_tile_emul.cpp"}


# ------------------------------------------------------------------ rows
def rows(vals):
    return np.array([pm.limbs(v) for v in vals], dtype=np.uint64).reshape(len(vals), 5)


def value(r):
    return sum((int(w) & M52) << (52 * i) for i, w in enumerate(r))


def pt_rows(pts):
    return np.array([sum(pm.pt_limbs(q), []) for q in pts], dtype=np.uint64).reshape(len(pts), 20)


def row_pt(r):
    return tuple(value(r[5 * c:5 * c + 5]) for c in range(4))


def enc_rows(vals):
    """256-bit integers (or 32-byte strings) -> (n, 32) uint8."""
    b = b"".join(v if isinstance(v, bytes) else int(v).to_bytes(32, "little") for v in vals)
    return np.frombuffer(b, dtype=np.uint8).reshape(len(vals), 32).copy()


def flags(xs):
    return np.array([1 if x else 0 for x in xs], dtype=np.uint8)


def affine_rows(arr):
    """(n, 20) extended points -> (n, 10) affine limbs; a row with Z = 0 or T Z != X Y becomes all ones."""
    out = []
    for r in np.asarray(arr).reshape(-1, 20):
        x, y, z, t = (v % P for v in row_pt(r))
        if z == 0 or (t * z - x * y) % P:
            out.append([M52] * 10)
        else:
            zi = pow(z, -1, P)
            out.append(pm.limbs(x * zi % P) + pm.limbs(y * zi % P))
    return np.array(out, dtype=np.uint64)


def affine_of(pts):
    return np.array([pm.limbs(a) + pm.limbs(b) for a, b in (pm.ed_affine(q) for q in pts)], dtype=np.uint64)


def scaled(q, lam):
    return tuple(c * lam % P for c in q)


def some_points(n, seed):
    """n subgroup points k B in non-trivial extended coordinates (Z != 1)."""
    rng = random.Random(seed)
    return [scaled(pm.ed_scalar_mul(pm.BASEPOINT, rng.randrange(1, L)), rng.randrange(2, P)) for _ in range(n)]


class Case:
    """op(ins; params) must give `want`.  cmp: "exact" (every output limb / byte) or "group" (output 0 holds points: the same
    affine point with T Z = X Y).  ok: index of the accept flag among the outputs -- rows it rejects compare the flag only.
    rowwise: row i of the outputs depends on row i of the inputs alone, so the case can be tiled to any batch size."""

    def __init__(self, op, ins, want, cmp="exact", ok=None, rowwise=True, **params):
        self.op, self.ins, self.want, self.cmp, self.ok, self.rowwise, self.params = op, tuple(ins), tuple(want), cmp, ok, rowwise, params
        n = len(self.ins[0])
        assert all(x is None or len(x) == n for x in self.ins) and (not rowwise or all(len(w) == n for w in self.want)), op

    def label(self):
        return "%s%s" % (self.op, sorted(self.params.items()) if self.params else "")

    def tiled(self, n, shift=0):
        """The same rows repeated (from row `shift` on) to a batch of n."""
        assert self.rowwise
        idx = (np.arange(n) + shift) % len(self.ins[0])
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.ins = tuple(None if x is None else np.ascontiguousarray(x[idx]) for x in self.ins)
        c.want = tuple(np.ascontiguousarray(w[idx]) for w in self.want)
        return c

    def _compared(self, got):
        """(output index, got, want, row numbers) per output, as they are compared: points as affine limbs under cmp="group",
        the rows the accept flag rejects dropped from every output but the flag."""
        keep = None
        if self.ok is not None:
            keep = np.asarray(self.want[self.ok]).astype(bool)
        for i, (g, w) in enumerate(zip(got, self.want)):
            g, w = np.asarray(g), np.asarray(w)
            if self.cmp == "group" and i == 0:
                g = affine_rows(g)
            g = g.reshape(w.shape) if g.size == w.size else g
            at = np.arange(len(w))
            if keep is not None and i != self.ok:
                g, w, at = g[keep], w[keep], at[keep]
            yield i, g, w, at

    def mismatches(self, got):
        """Indices of the outputs that differ from `want`."""
        return [i for i, g, w, _ in self._compared(got) if g.shape != w.shape or not np.array_equal(g.astype(w.dtype), w)]

    def bad_rows(self, got, output=None):
        """Sorted indices of the rows that differ from `want` in any output (or in output `output` alone), by the rules of
        `mismatches`; an output of another shape than expected counts with every row it is compared on."""
        bad = set()
        for i, g, w, at in self._compared(got):
            if output is not None and i != output:
                continue
            if g.shape != w.shape:
                bad.update(at.tolist())
            else:
                differ = (g.astype(w.dtype) != w).reshape(len(w), -1).any(axis=1)
                bad.update(at[differ].tolist())
        return sorted(bad)


# ------------------------------------------------------------------ the product form of a wave (mulmod cases)
WAVE = 64
TOPBIT = {0: 252, 1: 249}                    # modl -> F::TOPBIT of zc_arith.hip.h: operands below 2^TOPBIT take the one-pass product
MAX_LEVEL = 3


def mulmod_levels(case, which):
    """Per row of a mulmod case, how far its operands reach above 2^TOPBIT, read from the limbs as fe_mulmod_limbs52 /
    fe_sqrmod_limbs52 do (bits of limb 4 from TOPBIT - 208 on; the product ORs both operands, the square looks at `a` alone):
    0 = eligible for the one-pass form, k = the highest set bit is TOPBIT + k - 1 (capped at MAX_LEVEL).  which: "mul" / "sq"."""
    assert case.op == "mulmod" and which in ("mul", "sq")
    a, b = (np.asarray(x, dtype=np.uint64) for x in case.ins)
    top = (a[:, 4] | b[:, 4]) if which == "mul" else a[:, 4]
    top = (top & np.uint64(M52)) >> np.uint64(TOPBIT[case.params["modl"]] - 208)
    return np.array([min(int(t).bit_length(), MAX_LEVEL) for t in top])


def wave_levels(levels):
    """The wave model: a wave is WAVE consecutive rows of one call, and the device chooses the product form with a ballot over
    it.  Per row, the highest level in the row's wave -- the wave takes the one-pass form exactly when that is 0."""
    levels = np.asarray(levels)
    out = np.empty_like(levels)
    for w in range(0, len(levels), WAVE):
        out[w:w + WAVE] = levels[w:w + WAVE].max()
    return out


def _pad_wave(idx):
    """idx repeated from its start up to a whole number of waves."""
    idx = list(idx)
    return idx + [idx[j % len(idx)] for j in range(-len(idx) % WAVE)]


def pack_order(levels, packing):
    """Row order of one packing of a mulmod case (indices into the case, every row at least once).
    "one-pass": the rows of each level in whole waves of their own, the last wave of a level filled with repeats of that
    level's rows -- so every eligible row (level 0) sits in an all-eligible wave, the ineligible rows follow in waves without
    an eligible row, and a wave of rows just above 2^TOPBIT holds no row further up (a threshold moved by a bit shows there).
    "two-pass": 63 eligible rows and one ineligible row per wave, the ineligible rows taking turns; the last wave holds what
    is left of both -- so every eligible row meets the two Montgomery passes."""
    levels = np.asarray(levels)
    elig, inel = np.flatnonzero(levels == 0).tolist(), np.flatnonzero(levels > 0).tolist()
    assert elig and inel
    if packing == "one-pass":
        return np.array(sum((_pad_wave(np.flatnonzero(levels == lv)) for lv in range(MAX_LEVEL + 1) if (levels == lv).any()), []))
    assert packing == "two-pass"
    order, used = [], 0
    for s in range(0, len(elig), WAVE - 1):
        order += elig[s:s + WAVE - 1] + [inel[used % len(inel)]]
        used += 1
    return np.array(order + inel[used:])


def packed(case, which, packing):
    """(the mulmod case reordered by pack_order for the product ("mul") or the square ("sq"), `want` alike; the order)."""
    order = pack_order(mulmod_levels(case, which), packing)
    c = Case.__new__(Case)
    c.__dict__.update(case.__dict__)
    c.ins = tuple(np.ascontiguousarray(x[order]) for x in case.ins)
    c.want = tuple(np.ascontiguousarray(w[order]) for w in case.want)
    return c, order


def run(family, backend, cases=None):
    """The failed comparisons of one family on one backend, as labels; [] = every comparison the backend can make passed."""
    failed, made = [], 0
    for case in (FAMILIES[family].cases() if cases is None else cases):
        got = backend.call(case)
        if got is None:
            continue
        made += 1
        bad = case.mismatches(got)
        if bad:
            failed.append("%s: outputs %s" % (case.label(), bad))
    assert made > 0, "family %s: the backend ran nothing" % family
    return failed


# ------------------------------------------------------------------ the host-emulation backend
def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _out(n, w, dt=np.uint64):
    return np.zeros((n, w) if w else (n,), dtype=dt)


def _words(b):
    return np.ascontiguousarray(b).view(np.uint64).reshape(len(b), 4)


class EmulBackend:
    def __init__(self, lib):
        self.lib = lib

    def call(self, case):
        fn = getattr(self, "op_" + case.op, None)
        if fn is None:
            return None
        ins = [None if x is None else np.ascontiguousarray(x) for x in case.ins]
        return fn(len(ins[0]), *ins, **case.params)

    def _has(self, name):
        return hasattr(self.lib, name)

    def op_mulmod(self, n, a, b, modl):
        prod, sq = _out(n, 5), _out(n, 5)
        self.lib.emul_mulmod(_p(a), _p(b), _p(prod), _p(sq), C.c_size_t(n), modl)
        return prod, sq

    def op_mul_ilp(self, n, a, b):
        prod, sq = _out(n, 5), _out(n, 5)
        self.lib.emul_fe_mul_square_ilp(_p(a), _p(b), _p(prod), _p(sq), C.c_size_t(n))
        return prod, sq

    def op_fe_invert(self, n, a, c=0, lone=False):
        out, ok = _out(n, 5), _out(n, 0, np.uint8)
        if c == 0:
            self.lib.emul_fe_invert(_p(a), _p(out), _p(ok), C.c_size_t(n))
        else:
            (self.lib.emul_fe_invert_chunked_lone if lone else self.lib.emul_fe_invert_chunked)(_p(a), _p(out), _p(ok), C.c_size_t(n), c)
        return out, ok

    def op_fe_div(self, n, num, den, c=2, lone=False):
        out, ok = _out(n, 5), _out(n, 0, np.uint8)
        (self.lib.emul_fe_div_chunked_lone if lone else self.lib.emul_fe_div_chunked)(_p(num), _p(den), _p(out), _p(ok), C.c_size_t(n), c)
        return out, ok

    def op_ed_to_affine(self, n, pts, c=0):
        xy, ok = _out(n, 10), _out(n, 0, np.uint8)
        if c == 0:
            self.lib.emul_ed_to_affine(_p(pts), _p(xy), _p(ok), C.c_size_t(n))
        else:
            self.lib.emul_ed_to_affine_chunked(_p(pts), _p(xy), _p(ok), C.c_size_t(n), c)
        return xy, ok

    def op_sqrt_ratio_i(self, n, u, v):
        out, sq = _out(n, 5), _out(n, 0, np.uint8)
        self.lib.emul_fe_sqrt_ratio_i(_p(u), _p(v), _p(out), _p(sq), C.c_size_t(n))
        return out, sq

    def op_fe_is_positive(self, n, a):
        out = _out(n, 0, np.uint8)
        self.lib.emul_fe_is_positive(_p(a), _p(out), C.c_size_t(n))
        return (out,)

    def op_fe_mod_sqrt(self, n, a, sign):
        out, ok = _out(n, 5), _out(n, 0, np.uint8)
        self.lib.emul_fe_mod_sqrt(_p(a), sign, _p(out), _p(ok), C.c_size_t(n))
        return out, ok

    def _unary(self, name, n, *ins):
        out = _out(n, 5)
        getattr(self.lib, name)(*[_p(x) for x in ins], _p(out), C.c_size_t(n))
        return (out,)

    def op_fe_half(self, n, a): return self._unary("emul_fe_half", n, a)
    def op_sc_half(self, n, a): return self._unary("emul_sc_half", n, a)
    def op_fe_pow(self, n, a, e): return self._unary("emul_fe_pow", n, a, e)
    def op_sc_pow(self, n, a, e): return self._unary("emul_sc_pow", n, a, e)

    def op_fe_legendre(self, n, a, rounds=40):
        jac, pw = _out(n, 0, np.uint8), _out(n, 0, np.uint8)
        self.lib.emul_fe_legendre(_p(a), _p(jac), _p(pw), C.c_size_t(n), rounds)
        return jac, pw

    def op_sc_invert(self, n, a, c=0, lone=False):
        out, ok = _out(n, 5), _out(n, 0, np.uint8)
        if self._has("emul_sc_invert_row"):                                # emul.cpp: the row function only
            if c:
                return None
            self.lib.emul_sc_invert_row(_p(a), _p(out), _p(ok), C.c_size_t(n))
        elif c == 0:
            self.lib.emul_sc_invert(_p(a), _p(out), _p(ok), C.c_size_t(n))
        else:
            self.lib.emul_sc_invert_chunked(_p(a), _p(out), _p(ok), C.c_size_t(n), c, 1 if lone else 0)
        return out, ok

    def op_sc_reduce(self, n, b):
        out = _out(n, 5)
        (self.lib.emul_sc_from_bytes_wide if b.shape[1] == 64 else self.lib.emul_sc_from_bytes_mod_order)(_p(b), _p(out), C.c_size_t(n))
        return (out,)

    def op_sc_muladd(self, n, a, b, c):
        out = _out(n, 5)
        self.lib.emul_sc_muladd(_p(a), _p(b), _p(c), _p(out), C.c_size_t(n))
        return (out,)

    def op_ed_add_plain(self, n, a, b, mode):
        out = _out(n, 20)
        self.lib.emul_ed_add_plain(_p(a), _p(b), _p(out), C.c_size_t(n), mode)
        return (out,)

    def op_ed_scalar_mul(self, n, pts, k, how):
        out = _out(n, 20)
        if how in ("ltr", "naf"):
            self.lib.emul_ed_scalar_mul_mode(_p(pts), _p(k), _p(out), C.c_size_t(n), 1 if how == "ltr" else 2)
        else:
            name = {"strict": "emul_ed_scalar_mul", "small": "emul_ed_scalar_mul_small", "fast": "emul_ed_scalar_mul_fast"}[how]
            getattr(self.lib, name)(_p(pts), _p(k), _p(out), C.c_size_t(n))
        return (out,)

    def op_bucket_sum(self, n, pts):
        out = _out(1, 20)
        self.lib.emul_bucket_sum(_p(pts), C.c_size_t(n), _p(out))
        return (out,)

    def op_ed_compress(self, n, pts):
        enc, ok = _out(n, 4), _out(n, 0, np.uint8)
        self.lib.emul_ed_compress(_p(pts), _p(enc), _p(ok), C.c_size_t(n))
        return enc.view(np.uint8).reshape(n, 32), ok

    def op_ris_compress(self, n, pts):
        enc = _out(n, 4)
        self.lib.emul_ris_compress(_p(pts), _p(enc), C.c_size_t(n))
        return (enc.view(np.uint8).reshape(n, 32),)

    def _decode(self, name, n, b):
        out, ok = _out(n, 20), _out(n, 0, np.uint8)
        getattr(self.lib, name)(_p(_words(b)), _p(out), _p(ok), C.c_size_t(n))
        return out, ok

    def op_ed_decompress(self, n, b): return self._decode("emul_ed_decompress", n, b)
    def op_ris_decompress(self, n, b): return self._decode("emul_ris_decompress", n, b)

    def _flag2(self, name, n, a, b):
        out = _out(n, 0, np.uint8)
        getattr(self.lib, name)(_p(a), _p(b), _p(out), C.c_size_t(n))
        return (out,)

    def op_ed_eq(self, n, a, b): return self._flag2("emul_ed_eq", n, a, b)
    def op_ris_eq(self, n, a, b): return self._flag2("emul_ris_eq", n, a, b)

    def op_ed_is_valid(self, n, a):
        out = _out(n, 0, np.uint8)
        self.lib.emul_ed_is_valid(_p(a), _p(out), C.c_size_t(n))
        return (out,)

    def op_ris_elligator(self, n, r0):
        out = _out(n, 20)
        self.lib.emul_ris_elligator(_p(r0), _p(out), C.c_size_t(n))
        return (out,)

    def op_scalar_effective(self, n, k):
        eff, nbits = _out(n, 5), _out(n, 0, np.int32)
        self.lib.emul_scalar_effective(_p(k), _p(eff), _p(nbits), C.c_size_t(n))
        return eff, nbits

    def op_digits(self, n, k, radix):
        cnt = 66 if radix == 16 else 33
        rec, sto, tops = _out(n, cnt, np.int8), _out(n, cnt, np.int8), _out(n, 2, np.int32)
        (self.lib.emul_lincomb_digits if radix == 16 else self.lib.emul_base_digits)(_p(k), _p(rec), _p(sto), _p(tops), C.c_size_t(n))
        return rec, sto, tops

    def op_ed_lincomb(self, n, pts, k):
        out = _out(n, 20)
        assert self.lib.emul_ed_lincomb(_p(pts), _p(k), C.c_size_t(pts.shape[1]), _p(out), C.c_size_t(n), None, None) == 0
        return (out,)

    def op_ed_mul_base(self, n, k):
        out = _out(n, 20)
        self.lib.emul_ed_mul_base(_p(k), _p(out), C.c_size_t(n))
        return (out,)

    def op_ris_lincomb(self, n, enc, k, kb):
        out, ok = _out(n, 32, np.uint8), _out(n, 0, np.uint8)
        assert self.lib.emul_ris_lincomb(_p(enc), _p(k), C.c_size_t(enc.shape[1]), _p(kb), _p(out), _p(ok), C.c_size_t(n), None) == 0
        return out, ok

    def op_sm_tiles(self, n, pts, k, steps=None):
        out, st = _out(n, 20), _out((n + 63) // 64, 3, np.int32)
        self.lib.emul_sm_tiles(_p(pts), _p(k), _p(out), C.c_size_t(n), _p(st), 1)
        return (out,) if steps is None else (out, st)


# ------------------------------------------------------------------ the Engine backend (GPU tier)
STRICT_OPS = ("ed_scalar_mul", "sm_tiles")
# zc::LaunchForm (dusk_zerocaf_amd/csrc/zc_launch_plan.h) in the header's order; tests/test_launch_plan_emul.py keeps it so
LAUNCH_FORMS = ("per_lane", "staged", "strict_quad", "strict_small", "strict_block", "strict_pw", "strict_pw_unified", "inv_per_element", "inv_chunked", "inv_lone")


class Form:
    """One launch form of an operation that has several (tests/test_gpu_kill_vector_forms.py holds the table).  ops: the case
    operations it is a form of.  lo, hi: the batch sizes that reach it (inclusive).  env: the ZC_* knobs the engine's context
    must have been created under.  hooks: the engine runs the test-hooks build.  staged: whether every launch of the call takes
    its LDS-staged kernel (None: the operation has no such kernel) -- checked against the test build's launch counter where
    the engine has one.  misalign: rows 8 bytes off a 16-byte boundary.  small: the independent-chain strict kernel, the one
    how="small" names.  launch: the name of the zc::LaunchForm (LAUNCH_FORMS above) every call must be exactly
    one launch of, by the test build's per-form counters (None: not checked)."""

    def __init__(self, name, ops, lo=1, hi=1 << 40, env=None, hooks=False, staged=None, misalign=False, small=False, launch=None):
        self.name, self.ops, self.lo, self.hi, self.env = name, tuple(ops), lo, hi, dict(env or {})
        self.hooks, self.staged, self.misalign, self.small, self.launch = hooks, staged, misalign, small, launch


class EngineBackend:
    """The same cases through the C ABI.  chunk: the ZC_INV_CHUNK the engine's context was created under (None: the library's
    default) -- an inversion case runs on the engine whose chunk it names, every other case on the default engine only.
    device: inputs as torch tensors on the GPU.  misalign: arrays that start 8 bytes off a 16-byte boundary.
    form: a `Form` -- only the cases of its operations run (the others have one form: None), at a batch size inside its range,
    on device tensors so that one call is one launch; `how="small"` runs where the form is that kernel.  Per call, `counted`
    collects (op, staged launches counted by the test build or None) and `forms` (op, {form name: launches} for the forms of
    zc_launch_plan.h that the call launched, or None without the test build)."""

    def __init__(self, engine, chunk=None, device=False, misalign=False, form=None):
        self.e, self.chunk, self.device, self.misalign, self.form = engine, chunk, device, misalign, form
        self.counted, self.forms = [], []
        if form is not None:
            self.device, self.misalign = True, form.misalign

    def _in(self, a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        if self.device:
            import torch
            t = torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a)
            if self.misalign:
                raw = torch.empty(t.numel() * t.element_size() + 16, dtype=torch.uint8, device="cuda")
                view = raw[8:8 + t.numel() * t.element_size()].view(t.dtype).view(t.shape)
                view.copy_(t)
                assert raw.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 8 and view.is_contiguous()
                return view
            return t.cuda()
        if self.misalign:
            raw = np.zeros(a.nbytes + 32, dtype=np.uint8)
            off = (8 - raw.ctypes.data) % 16
            view = raw[off:off + a.nbytes].view(a.dtype).reshape(a.shape)
            view[...] = a
            assert view.ctypes.data % 16 == 8
            return view
        return a

    @classmethod
    def reach(cls, case):
        """Indices of the outputs of `case` that an EngineBackend of some configuration (chunk, form) returns: () where the C ABI
        has no such operation or setting -- digit strings, step counts, a lone-chunk multiplier, a Jacobi schedule of its own."""
        if not hasattr(cls, "op_" + case.op) or case.params.get("lone") or (case.op == "fe_legendre" and case.params.get("rounds", 40) != 40):
            return ()
        return (0,) if case.op == "sm_tiles" else tuple(range(len(case.want)))

    @staticmethod
    def _host(x):
        if hasattr(x, "cpu"):
            x = x.cpu().numpy()
            if x.dtype == np.int64:
                x = x.view(np.uint64)
        return x

    def takes(self, case):
        """Under a form: is `case` one of the form's operations in a setting that has that form?"""
        if self.form is None:
            return True
        how = case.params.get("how", "strict")
        return case.op in self.form.ops and (case.op not in STRICT_OPS or how == "strict" or (how == "small" and self.form.small))

    def call(self, case):
        fn = getattr(self, "op_" + case.op, None)
        if fn is None or not self.takes(case):
            return None
        inv = case.op in ("fe_invert", "fe_div", "ed_to_affine", "sc_invert")
        c = case.params.get("c", 0)
        if inv:
            if case.params.get("lone") or (c or None) != self.chunk:
                return None
        elif self.chunk is not None:
            return None
        if self.form is not None:
            n = len(case.ins[0])
            assert self.form.lo <= n <= self.form.hi, "%s: %d rows do not reach the form '%s'" % (case.label(), n, self.form.name)
        c0 = self._launch_forms()
        got = fn(*[self._in(x) for x in case.ins], **{k: v for k, v in case.params.items() if k not in ("c", "lone")})
        if got is None:
            return None
        delta = None if c0 is None else {f: b - a for f, a, b in zip(LAUNCH_FORMS, c0, self._launch_forms()) if b != a}
        self.counted.append((case.op, None if delta is None else delta.get("staged", 0)))
        self.forms.append((case.op, delta))
        return tuple(self._host(x) for x in (got if isinstance(got, tuple) else (got,)))

    def _launch_forms(self):
        """The test build's launch counters per form of zc_launch_plan.h (None: the engine runs the product)."""
        hook = getattr(self.e.lib, "zc_test_launch_forms", None)
        if hook is None:
            return None
        counts = (C.c_uint64 * len(LAUNCH_FORMS))()
        assert hook(self.e.ctx, counts, len(counts)) == 0
        return list(counts)

    def op_mulmod(self, a, b, modl):
        return (self.e.sc_mul(a, b), self.e.sc_square(a)) if modl else (self.e.fe_mul(a, b), self.e.fe_square(a))

    def op_fe_invert(self, a): return self.e.fe_invert(a)
    def op_fe_div(self, num, den): return self.e.fe_div(num, den)
    def op_ed_to_affine(self, pts): return self.e.ed_to_affine(pts)
    def op_sc_invert(self, a): return self.e.sc_invert(a)
    def op_sqrt_ratio_i(self, u, v): return self.e.fe_sqrt_ratio_i(u, v)
    def op_fe_is_positive(self, a): return self.e.fe_is_positive(a)
    def op_fe_mod_sqrt(self, a, sign): return self.e.fe_mod_sqrt(a, sign)
    def op_fe_half(self, a): return self.e.fe_half(a)
    def op_sc_half(self, a): return self.e.sc_half(a)
    def op_fe_pow(self, a, e): return self.e.fe_pow(a, e)
    def op_sc_pow(self, a, e): return self.e.sc_pow(a, e)

    def op_fe_legendre(self, a, rounds=40):
        if rounds != 40:
            return None
        f = self.e.fe_legendre_symbol(a)
        return f, f

    def op_sc_reduce(self, b): return self.e.sc_from_bytes_wide(b) if b.shape[1] == 64 else self.e.sc_from_bytes_mod_order(b)
    def op_sc_muladd(self, a, b, c): return self.e.sc_muladd(a, b, c)

    def op_ed_add_plain(self, a, b, mode):
        return self.e.ed_add(a, b) if mode == 0 else self.e.ed_sub(a, b) if mode == 1 else self.e.ed_double(a)

    def op_ed_scalar_mul(self, pts, k, how):
        if how == "small":                                  # the strict call at a batch size that takes k_ed_scalar_mul_small
            return self.e.ed_scalar_mul(pts, k, flags=0) if self.form is not None and self.form.small else None
        return self.e.ed_scalar_mul(pts, k, flags={"strict": 0, "ltr": 1, "naf": 2, "fast": 16}[how])

    def op_sm_tiles(self, pts, k, steps=None): return self.e.ed_scalar_mul(pts, k, flags=0)
    def op_ed_compress(self, pts): return self.e.ed_compress(pts)
    def op_ris_compress(self, pts): return self.e.ris_compress(pts)
    def op_ed_decompress(self, b): return self.e.ed_decompress(b)
    def op_ris_decompress(self, b): return self.e.ris_decompress(b)
    def op_ed_eq(self, a, b): return self.e.ed_eq(a, b)
    def op_ris_eq(self, a, b): return self.e.ris_eq(a, b)
    def op_ed_is_valid(self, a): return self.e.ed_is_valid(a)
    def op_ris_elligator(self, r0): return self.e.ris_elligator(r0)
    def op_ed_lincomb(self, pts, k): return self.e.ed_lincomb(pts, k)
    def op_ed_mul_base(self, k): return self.e.ed_mul_base(k)
    def op_ris_lincomb(self, enc, k, kb): return self.e.ris_lincomb(enc, k, kb)


# ------------------------------------------------------------------ expected values
def want_invert(a, mod):
    vals = [value(r) % mod for r in a]
    return rows([pow(v, -1, mod) if v else 0 for v in vals]), flags(vals)


def want_div(num, den):
    d = [value(r) % P for r in den]
    return rows([value(x) * pow(v, -1, P) % P if v else 0 for x, v in zip(num, d)]), flags(d)


def want_affine(pts):
    xy, ok = [], []
    for r in pts:
        x, y, z, _ = (v % P for v in row_pt(r))
        zi = pow(z, -1, P) if z else 0
        xy.append(pm.limbs(x * zi % P) + pm.limbs(y * zi % P))
        ok.append(1 if z else 0)
    return np.array(xy, dtype=np.uint64), np.array(ok, dtype=np.uint8)


def want_points(pts):
    """Model results (None = rejected) -> (rows, ok)."""
    return pt_rows([q if q is not None else pm.IDENT for q in pts]), flags(q is not None for q in pts)


def inversion_cases(a, mod):
    """One batch through every form of the shared inversion: one row per lane, c rows per lane on both multipliers."""
    op = "fe_invert" if mod == P else "sc_invert"
    want = want_invert(a, mod)
    out = [Case(op, [a], want, ok=1)]
    for c in INV_CHUNKS:
        out += [Case(op, [a], want, ok=1, c=c), Case(op, [a], want, ok=1, c=c, lone=True)]
    return out


def effective(v):
    """The integer double_and_add multiplies by for the 260-bit pattern v (zc_curve.hip.h: scalar_effective)."""
    t = 0
    while (v >> t) % (1 << 256):
        t += 1
    return v % (1 << t), t


def signed_digits(v, width, count):
    """Signed radix-2^width digits of effective(v), in [-2^(width-1), 2^(width-1)), and the index of the highest non-zero one."""
    v, carry, out = effective(v)[0], 0, []
    for i in range(count):
        d = ((v >> (width * i)) & ((1 << width) - 1)) + carry
        carry = 1 if d >= 1 << (width - 1) else 0
        out.append(d - (carry << width))
    assert carry == 0
    return out, max([i for i, d in enumerate(out) if d] or [-1])


# ------------------------------------------------------------------ families
class Family:
    def __init__(self, lib, build, doc):
        self.lib, self._build, self.doc, self._cases = lib, build, doc, None

    def cases(self):
        if self._cases is None:
            self._cases = self._build()
        return self._cases


def _field_edges(mod, top):
    e = [0, 1, 2, mod - 1, mod - 2, (mod - 1) // 2, (mod + 1) // 2, (1 << top) - 1, 1 << (top - 1), mod - (1 << 60), (1 << top) - (1 << 125),
         (1 << 125) - 1, 1 << 125, (1 << 232) - 1, 1 << 232, (1 << 29) - 1, 1 << 29, (1 << 261) % mod]
    return e + [((1 << 29 * k) - 1) % mod for k in range(2, 9)] + [((1 << top) - 1) ^ (1 << i) for i in range(0, top, 29)]


def build_field_core():
    rng = random.Random(SEED + 1)
    cases = []
    for modl, mod, top in ((0, P, 252), (1, L, 249)):
        e = _field_edges(mod, top)
        canon = e + [rng.randrange(mod) for _ in range(160)]
        raw = [1 << top, (1 << top) + 1, mod, mod + 1, (1 << 260) - 1, 255 * mod if mod == P else 2047 * mod] + [rng.getrandbits(260) for _ in range(60)]
        raw += [(2 << top) - 1, (2 << top) - (1 << 100), (2 << top) - (1 << 200)] + [(1 << top) | rng.getrandbits(top) for _ in range(13)]   # just above the one-pass range
        raw += [(4 << top) - 1, (4 << top) - (1 << 100)] + [(2 << top) | rng.getrandbits(top + 1) for _ in range(14)]                        # ... and one bit further
        a = canon + e + raw + canon[:len(raw)]
        b = canon[::-1] + [e[(7 * i + 3) % len(e)] for i in range(len(e))] + raw[::-1] + raw
        cases.append(Case("mulmod", [rows(a), rows(b)], [rows([x * y % mod for x, y in zip(a, b)]), rows([x * x % mod for x in a])], modl=modl))
    a = _field_edges(P, 252) + [rng.randrange(P) for _ in range(60)]
    b = a[::-1]
    cases.append(Case("mul_ilp", [rows(a), rows(b)], [rows([x * y % P for x, y in zip(a, b)]), rows([x * x % P for x in a])]))
    for op, mod in (("fe_half", P), ("sc_half", L)):
        a = [0, 1, 2, 3, mod - 1, mod - 2, (mod - 1) // 2, (mod + 1) // 2] + [rng.randrange(mod) for _ in range(24)]
        cases.append(Case(op, [rows(a)], [rows([x * ((mod + 1) // 2) % mod for x in a])]))
    for op, mod in (("fe_pow", P), ("sc_pow", L)):
        a = [2, 3, mod - 1, rng.randrange(mod), rng.randrange(mod), 0, 5, 7] + [rng.randrange(mod) for _ in range(8)]
        e = [0, 1, 2, mod - 2, mod - 1, 5, (mod - 1) // 2, (1 << 248) + 1] + [rng.randrange(mod) for _ in range(8)]
        cases.append(Case(op, [rows(a), rows(e)], [rows([pow(x, y, mod) for x, y in zip(a, e)])]))
    a = rows([1, 2, P - 1, P - 2, HALF, HALF + 1, 0, 1 << 251, 3] + [rng.randrange(1, P) for _ in range(40)])
    cases += inversion_cases(a, P)
    num = rows([rng.randrange(P) for _ in range(len(a))])
    for c in INV_CHUNKS:
        cases += [Case("fe_div", [num, a], want_div(num, a), ok=1, c=c), Case("fe_div", [num, a], want_div(num, a), ok=1, c=c, lone=True)]
    s = np.concatenate([S.invert_edges(), np.array([w for _, w in S.zero_patterns()], dtype=np.uint64), S.random_invert_rows(24, SEED + 2)])
    cases.append(Case("sc_invert", [s], want_invert(s, L), ok=1))
    vals = [rng.randrange(1, P) for _ in range(48)] + [x * x % P for x in (rng.randrange(1, P) for _ in range(16))] + [0, 1, 2, 6, P - 1, 1 << 200]
    want = flags(pm.legendre(v) for v in vals)
    assert 8 < int(want.sum()) < len(vals) - 8
    cases += [Case("fe_legendre", [rows(vals)], [want, want], rounds=r) for r in (40, 3)]
    u = [rng.randrange(1, P) for _ in range(48)] + [0, 5, 0, 1, 1]
    v = [rng.randrange(1, P) for _ in range(48)] + [7, 0, 0, 1, P - 1]
    res = [pm.sqrt_ratio_i(x, y) for x, y in zip(u, v)]
    assert 8 < sum(r[0] for r in res) < 44
    cases.append(Case("sqrt_ratio_i", [rows(u), rows(v)], [rows([r[1] for r in res]), flags(r[0] for r in res)]))
    return cases


def build_group_core():
    rng = random.Random(SEED + 10)
    pts = some_points(24, SEED + 11)
    A, B = pts[:12], pts[12:]
    A[0], B[1], B[2] = pm.IDENT, pm.IDENT, A[2]
    cases = []
    for mode, f in ((0, lambda a, b: pm.ed_add(a, b)), (1, lambda a, b: pm.ed_sub(a, b)), (2, lambda a, b: pm.ed_add(a, a))):
        cases.append(Case("ed_add_plain", [pt_rows(A), pt_rows(B)], [pt_rows([f(a, b) for a, b in zip(A, B)])], mode=mode))
    ks = [0, 1, 2, 3, 8, L - 1, L, (1 << 249) - 1, 1 << 248, (1 << 252) - 1, (1 << 260) - 1, 1 << 255] + [rng.getrandbits(252) for _ in range(12)]
    Pk = pt_rows([pts[i % len(pts)] for i in range(len(ks))])
    strict = pt_rows([pm.ed_scalar_mul(row_pt(r), k) for r, k in zip(Pk, ks)])
    cases += [Case("ed_scalar_mul", [Pk, rows(ks)], [strict], how=how) for how in ("strict", "small")]
    cases.append(Case("ed_scalar_mul", [Pk, rows(ks)], [affine_rows(strict)], cmp="group", how="fast"))
    raw = V.raw_scalar_edges(8)
    cases.append(Case("scalar_effective", [raw], [rows([effective(value(r))[0] for r in raw]), np.array([effective(value(r))[1] for r in raw], dtype=np.int32)]))
    total = pm.IDENT
    for q in pts:
        total = pm.ed_add(total, q)
    cases.append(Case("bucket_sum", [pt_rows(pts)], [affine_of([total])], cmp="group", rowwise=False))
    # codecs: scaled representatives, the two x = 0 points, Z = 0, junk coordinates
    E = pts[:16] + [scaled(pm.IDENT, 12345), scaled((0, P - 1, 1, 0), 777)]
    junk = [tuple(rng.randrange(P) for _ in range(4)) for _ in range(12)] + [(A[3][0], A[3][1], 0, A[3][3])]
    wenc, wok = [], []
    for q in E + junk:
        try:
            if q[2] % P == 0:
                raise ZeroDivisionError
            y = pm.ed_affine(q)[1]
            den = (pm.D * y * y - pm.A) % P
            r = pm.mod_sqrt(pm.find_xx(y), 0) if den else None
            if r is None:
                raise ZeroDivisionError
            wenc.append(pm.ed_compress(q))
            wok.append(1)
        except (ZeroDivisionError, ValueError):
            wenc.append(bytes(32))
            wok.append(0)
    assert 0 < sum(wok[len(E):]) < len(junk) and all(wok[:len(E)])
    cases.append(Case("ed_compress", [pt_rows(E + junk)], [enc_rows(wenc), flags(wok)], ok=1))
    cases.append(Case("ris_compress", [pt_rows(E + junk[:12])], [enc_rows([pm.ris_compress(q) for q in E + junk[:12]])]))
    good = [b for b, k in zip(wenc, wok) if k]
    flipped = [bytes(b[:31]) + bytes([b[31] ^ 0x80]) for b in good[:8]]
    rnd = [bytes(rng.getrandbits(8) for _ in range(31)) + bytes([rng.getrandbits(4) | (rng.getrandbits(1) << 7)]) for _ in range(40)]
    dec = [pm.ed_decompress(b) for b in good + flipped + rnd]
    assert 8 < sum(q is not None for q in dec[len(good) + 8:]) < 32
    cases.append(Case("ed_decompress", [enc_rows(good + flipped + rnd)], want_points(dec), ok=1))
    renc = [pm.ris_compress(q) for q in E] + [bytes(rng.getrandbits(8) for _ in range(31)) + bytes([rng.getrandbits(3)]) for _ in range(40)]
    rdec = [pm.ris_decompress(b) for b in renc]
    assert all(q is not None for q in rdec[1:16]) and 4 < sum(q is not None for q in rdec[18:]) < 36
    cases.append(Case("ris_decompress", [enc_rows(renc)], want_points(rdec), ok=1))
    # equality: the same point rescaled, its negative, (x, -y), the four-torsion translate (i y, i x), Z = 0
    i_ = pm.SQRT_M1
    X = pts[:6]
    lhs, rhs, eq_ed, eq_ris = [], [], [], []
    for q in X:
        x, y, z, t = q
        for other in (scaled(q, 99), pm.ed_neg(q), (x, (-y) % P, z, (-t) % P), (i_ * y % P, i_ * x % P, z, (-t) % P), pts[7], (x, y, 0, t)):
            lhs.append(q)
            rhs.append(other)
            eq_ed.append(other[2] != 0 and pm.ed_eq(q, other))
            eq_ris.append(pm.ris_eq(q, other))
    for a, b in ((X[0], (0, 0, 0, 5)), ((0, 0, 0, 7), X[1]), ((0, 0, 0, 1), (0, 0, 0, 2))):    # Z = 0 and X = Y = 0: both cross products vanish
        lhs.append(a)
        rhs.append(b)
        eq_ed.append(False)
        eq_ris.append(pm.ris_eq(a, b))
    assert sum(eq_ed) == 6 and sum(a and not b for a, b in zip(eq_ris, eq_ed)) >= 12
    cases.append(Case("ed_eq", [pt_rows(lhs), pt_rows(rhs)], [flags(eq_ed)]))
    cases.append(Case("ris_eq", [pt_rows(lhs), pt_rows(rhs)], [flags(eq_ris)]))
    val = pts[:6] + [(q[0], q[1] ^ 1, q[2], q[3]) for q in pts[:3]] + [pm.IDENT, (1, 0, 1, 0)]
    wv = flags(((-x * x + y * y) * z * z - z ** 4 - pm.D * x * x * y * y) % P == 0 for x, y, z, _ in val)
    assert wv.tolist() == [1] * 6 + [0] * 3 + [1, 0]
    cases.append(Case("ed_is_valid", [pt_rows(val)], [wv]))
    r0 = [0, 1, 2, P - 1, HALF, HALF + 1] + [rng.randrange(P) for _ in range(26)]
    cases.append(Case("ris_elligator", [rows(r0)], [pt_rows([pm.elligator(r) for r in r0])]))
    tp = pt_rows(pts[:10] + [(A[3][0], A[3][1], 0, A[3][3])])
    cases.append(Case("ed_to_affine", [tp], want_affine(tp), ok=1))
    return cases


def ris_class(s):
    """Why ristretto.rs:96-154 accepts or rejects the canonical s: "ok", "nonsquare", "t negative", "y zero"."""
    ss = s * s % P
    u1, u2 = (1 - ss) % P, (1 + ss) % P
    v = (-(pm.D * u1 * u1) - u2 * u2) % P
    sq, i = pm.inv_sqrt(v * u2 * u2 % P)
    if not sq:
        return "nonsquare"
    dx = i * u2 % P
    x = 2 * s * dx % P
    x = x if pm.is_positive(x) else P - x
    y = u1 * (i * dx % P * v % P) % P
    return "t negative" if not pm.is_positive(x * y % P) else "y zero" if y == 0 else "ok"


def build_sign_boundaries():
    rng = random.Random(SEED + 20)
    cases = []
    b5 = [0, 1, HALF, HALF + 1, P - 1, HALF - 1, HALF + 2]
    cases.append(Case("fe_is_positive", [rows(b5)], [flags(pm.is_positive(v) for v in b5)]))
    # |r| through sqrt_ratio_i / inv_sqrt: u = r^2 v for a chosen root r on the boundary (square case) and u = r^2 v / i
    # (non-square case), so the value fp_abs sees is +-r
    u, v = [], []
    for r in (HALF, HALF + 1, 1, P - 1, HALF - 1, HALF + 2):
        for _ in range(4):
            d = rng.randrange(1, P)
            u += [r * r % P * d % P, r * r % P * d % P * pow(pm.SQRT_M1, -1, P) % P, 1]
            v += [d, d, pow(r * r % P, -1, P)]
    res = [pm.sqrt_ratio_i(x, y) for x, y in zip(u, v)]
    assert sum(r[1] == HALF for r in res) >= 16 and 0 < sum(r[0] for r in res) < len(res)
    cases.append(Case("sqrt_ratio_i", [rows(u), rows(v)], [rows([r[1] for r in res]), flags(r[0] for r in res)]))
    a = [0, 1, 4, HALF * HALF % P, (HALF + 1) ** 2 % P, 2, P - 1, 6] + [rng.randrange(P) for _ in range(16)]
    for sign in (0, 1):
        w = [pm.mod_sqrt(x, sign) for x in a]
        assert w[0] == 0 and 4 < sum(x is None for x in w) < 16
        cases.append(Case("fe_mod_sqrt", [rows(a)], [rows([x or 0 for x in w]), flags(x is not None for x in w)], ok=1, sign=sign))
    # encodings around (p - 1) / 2, at p and p + 1, with bit 255 set
    around = [HALF - d for d in range(12)] + [HALF + 1, HALF + 2, P, P + 1, P - 1, (1 << 255) | 2, (1 << 255) | (HALF - 6), (1 << 256) - 1, 1 << 252]
    ok_below = [s for s in around[:12] if ris_class(s) == "ok"]
    assert ok_below and ris_class(HALF) == "t negative"          # the nearest decodable s below the boundary; the boundary itself is rejected anyway
    rd = [pm.ris_decompress(s.to_bytes(32, "little")) for s in around]
    cases.append(Case("ris_decompress", [enc_rows(around)], want_points(rd), ok=1))
    ed_enc = []
    for y in (HALF, HALF + 1, P - 1, 1, 0, P, P + 1, HALF - 1):
        ed_enc += [y % (1 << 256), (y | (1 << 255)) % (1 << 256)]
    ed = [pm.ed_decompress(int(e).to_bytes(32, "little")) for e in ed_enc]
    assert sum(q is not None for q in ed) >= 6
    cases.append(Case("ed_decompress", [enc_rows(ed_enc)], want_points(ed), ok=1))
    # points whose encoding sits right below the boundary, and the torsion translates that must compress to the same bytes
    near = [pm.ris_decompress(s.to_bytes(32, "little")) for s in ok_below]
    i_ = pm.SQRT_M1
    cos = []
    for x, y, z, t in near:
        cos += [(x, y, z, t), ((-x) % P, (-y) % P, z, t), (i_ * y % P, i_ * x % P, z, (-t) % P), scaled((x, y, z, t), 3)]
    wenc = [pm.ris_compress(q) for q in cos]
    assert all(wenc[4 * j + c] == ok_below[j].to_bytes(32, "little") for j in range(len(near)) for c in range(4))
    cases.append(Case("ris_compress", [pt_rows(cos)], [enc_rows(wenc)]))
    return cases


def build_degenerate_encodings():
    rng = random.Random(SEED + 30)
    small = list(range(0, 48)) + [rng.randrange(HALF) for _ in range(40)]
    kinds = [ris_class(s) for s in small]
    assert kinds[0] == "ok" and kinds[1] == "y zero" and kinds.count("t negative") >= 8 and kinds.count("nonsquare") >= 8 and kinds.count("ok") >= 8
    rd = [pm.ris_decompress(s.to_bytes(32, "little")) for s in small]
    assert [q is not None for q in rd] == [k == "ok" for k in kinds]
    cases = [Case("ris_decompress", [enc_rows(small)], want_points(rd), ok=1)]
    # Edwards: x = 0 with and without the sign bit (y = 1, y = -1), y = 0, small y, non-residues
    ys = [1, P - 1, 0, 2, 3, 4, 5] + [rng.randrange(P) for _ in range(20)]
    enc = [y for y in ys] + [y | (1 << 255) for y in ys]
    ed = [pm.ed_decompress(int(e).to_bytes(32, "little")) for e in enc]
    assert ed[0] == (0, 1, 1, 0) and ed[len(ys)] == (0, 1, 1, 0) and 4 < sum(q is None for q in ed) < 40      # (y = p - 1 loses bit 252 to the 0x0F mask)
    cases.append(Case("ed_decompress", [enc_rows(enc)], want_points(ed), ok=1))
    # and back: x = 0 points in any scaling, both roots' signs
    back = [q for q in ed if q is not None]
    back = back + [scaled(q, rng.randrange(2, P)) for q in back]
    cases.append(Case("ed_compress", [pt_rows(back)], [enc_rows([pm.ed_compress(q) for q in back]), flags([1] * len(back))], ok=1))
    rback = [q for q in rd if q is not None]
    cases.append(Case("ris_compress", [pt_rows(rback)], [enc_rows([pm.ris_compress(q) for q in rback])]))
    return cases


def zero_by_value_rows(mod, top, kmax):
    """k N (zero), and its neighbours that are not: k N + 2^232 and k N + 2^(top - 1) keep the low eight 29-bit limbs of k N and
    change the ninth, k N +- 1 change the first."""
    zero, nonzero = [], []
    for k in (1, 2, kmax):
        zero.append(k * mod)
        nonzero += [k * mod + (1 << 232), k * mod + (1 << (top - 1)), k * mod + 1, k * mod - 1]
    assert all(v < 1 << 260 for v in zero + nonzero)
    return zero, nonzero


def _spread(special, filler, n):
    """n rows: the special rows at a stride that visits every position of a chunk of 2, 7 and 64, filler between them."""
    out = [filler[i % len(filler)] for i in range(n)]
    for j, s in enumerate(special):
        out[(j * 11) % n] = s
    return out


def build_zero_by_value_p():
    rng = random.Random(SEED + 40)
    zero, nonzero = zero_by_value_rows(P, 252, 255)
    fill = [rng.randrange(1, P) for _ in range(40)] + [(1 << 260) - 1, (1 << 260) - 2, (1 << 260) - 3]
    vals = _spread(zero + nonzero + [0, (1 << 260) - 1, (1 << 260) - 1], fill, 140)
    a = rows(vals)
    cases = inversion_cases(a, P)
    num = rows([rng.randrange(P) for _ in range(len(a))])
    for c in INV_CHUNKS:
        cases += [Case("fe_div", [num, a], want_div(num, a), ok=1, c=c), Case("fe_div", [num, a], want_div(num, a), ok=1, c=c, lone=True)]
    pts = pt_rows(some_points(7, SEED + 41))[np.arange(len(a)) % 7]
    pts[:, 10:15] = a                                                              # as the Z of a point
    cases += [Case("ed_to_affine", [pts], want_affine(pts), ok=1, c=c) for c in (0,) + INV_CHUNKS]
    return cases


def build_zero_by_value_l():
    rng = random.Random(SEED + 50)
    zero, nonzero = zero_by_value_rows(L, 249, 2047)
    fill = [rng.randrange(1, L) for _ in range(40)] + [(1 << 260) - 1, (1 << 260) - 2, (1 << 260) - 3]
    return inversion_cases(rows(_spread(zero + nonzero + [0, (1 << 260) - 1, (1 << 260) - 1], fill, 140)), L)


def divsteps_worst():
    with open(os.path.join(HERE, "golden", "divsteps_worst.json")) as f:
        return json.load(f)


def s_max():
    """The largest division-step count in tests/golden/divsteps_worst.json, over both moduli."""
    w = divsteps_worst()
    return max(w["s_max_p"], w["s_max_l"])


def build_longest_inversions_p():
    a = rows([int(e["a"], 16) for e in divsteps_worst()["p"]])
    cases = inversion_cases(a, P)
    pts = pt_rows(some_points(5, SEED + 60))[np.arange(len(a)) % 5]
    pts[:, 10:15] = a
    return cases + [Case("ed_to_affine", [pts], want_affine(pts), ok=1, c=c) for c in (0,) + INV_CHUNKS]


def build_longest_inversions_l():
    return inversion_cases(rows([int(e["a"], 16) for e in divsteps_worst()["l"]]), L)


def build_scalar_ext():
    cases = []
    for width in (64, 32):
        vals = S.reduction_values(width, 96, SEED + 70 + width)
        cases.append(Case("sc_reduce", [S.to_bytes(vals, width)], [S.canon_rows(vals)]))
    a, b, c = S.muladd_families(96, SEED + 71)
    cases.append(Case("sc_muladd", [a, b, c], [S.muladd_expected(a, b, c)]))
    top = [(1 << 249) - 1, (1 << 249) - 2, L - 1, 1 << 248, (1 << 125) - 1, 1 << 125, 0, 1]
    tri = [(x, y, z) for x in top for y in top[:4] for z in top[:3]]
    cases.append(Case("sc_muladd", [rows([t[0] for t in tri]), rows([t[1] for t in tri]), rows([t[2] for t in tri])], [rows([(x * y + z) % L for x, y, z in tri])]))
    return cases


def recoding_scalars():
    """Scalars whose signed 4-bit / 8-bit recodings carry out of the top digit, hold a single non-zero top window, or alternate
    between the extreme digits -- below L, below 2^256 and raw 260-bit patterns."""
    def rep(byte, n):
        return int.from_bytes(bytes([byte]) * n, "little")
    v = [rep(0x88, 31), rep(0x88, 32), rep(0x88, 32) | (0x8 << 256), (1 << 260) - 1, (1 << 252) - 8, (1 << 256) - 8, (1 << 249) - 8,
         rep(0xFF, 31), rep(0x80, 31), rep(0x80, 32), rep(0x08, 31), rep(0x08, 32), rep(0x87, 31), rep(0x78, 31), rep(0x86, 32), rep(0x7F, 32),
         0xF << 248, 0x8 << 248, 0x7 << 248, 0xFF << 248, 0x80 << 248, 0x7F << 248, 0xF << 252, 0x80 << 240, (0x8 << 256) | 9, (0xF << 256) | 1,
         8, 0x80, 0x88, 7, 0x7F, L - 1, L, 0]
    assert len(set(v)) == len(v) and all(x < 1 << 260 for x in v)
    return v


def _recoding_points(n, seed):
    pts = some_points(5, seed)
    return [pts[i % 5] for i in range(n)]


def _c_oracle():
    from oracle import zc_ref
    zc_ref.build()
    zc_ref.lib()
    return zc_ref


def build_recoding_fast():
    ks = recoding_scalars()
    pts = _recoding_points(len(ks), SEED + 80)
    Pk, K = pt_rows(pts), rows(ks)
    strict = pt_rows([pm.ed_scalar_mul(q, k) for q, k in zip(pts, ks)])
    cases = [Case("ed_scalar_mul", [Pk, K], [strict], how="strict"), Case("ed_scalar_mul", [Pk, K], [strict], how="small")]
    cases.append(Case("ed_scalar_mul", [Pk, K], [affine_rows(strict)], cmp="group", how="fast"))
    orc = _c_oracle()
    for how, mode in (("ltr", 1), ("naf", 2)):
        cases.append(Case("ed_scalar_mul", [Pk, K], [orc.ed_scalar_mul_mode(Pk, K, mode)], how=how))
    cases.append(Case("scalar_effective", [K], [rows([effective(k)[0] for k in ks]), np.array([effective(k)[1] for k in ks], dtype=np.int32)]))
    return cases


def _digit_case(ks, radix, count, width):
    dig = [signed_digits(k, width, count) for k in ks]
    d = np.array([x[0] for x in dig], dtype=np.int8)
    tops = np.array([[x[1], x[1]] for x in dig], dtype=np.int32)
    return Case("digits", [rows(ks)], [d, d, tops], radix=radix)


def build_recoding_lincomb():
    ks = recoding_scalars()
    cases = [_digit_case(ks, 16, 66, 4)]
    rng = random.Random(SEED + 90)
    for t in (1, 2, 3):
        n = len(ks)
        pts = [[q for q in _recoding_points(t, SEED + 91 + 7 * i)] for i in range(6)]
        prow = [pts[i % 6] for i in range(n)]
        krow = [[ks[(i + 5 * j) % n] if j != 1 else rng.getrandbits(249) for j in range(t)] for i in range(n)]
        want = []
        for pr, kr in zip(prow, krow):
            acc = pm.IDENT
            for q, k in zip(pr, kr):
                acc = pm.ed_add(acc, pm.ed_scalar_mul(q, k))
            want.append(acc)
        Pa = np.array([[sum(pm.pt_limbs(q), []) for q in pr] for pr in prow], dtype=np.uint64)
        Ka = np.array([[pm.limbs(k) for k in kr] for kr in krow], dtype=np.uint64)
        cases.append(Case("ed_lincomb", [Pa, Ka], [affine_of(want)], cmp="group"))
    return cases


def build_recoding_base():
    ks = recoding_scalars()
    cases = [_digit_case(ks, 256, 33, 8)]
    cases.append(Case("ed_mul_base", [rows(ks)], [affine_of([pm.ed_scalar_mul(pm.BASEPOINT, k) for k in ks])], cmp="group"))
    # the wire form: base term alone cannot stand (terms >= 1), so one decoded term with a recoding-edge scalar beside it
    n = len(ks)
    pts = _recoding_points(n, SEED + 100)
    enc = enc_rows([pm.ris_compress(q) for q in pts]).reshape(n, 1, 32)
    kt = [ks[(i + 3) % n] for i in range(n)]
    dec = [pm.ris_decompress(bytes(e[0])) for e in enc]
    want = [pm.ris_compress(pm.ed_add(pm.ed_scalar_mul(q, a), pm.ed_scalar_mul(pm.BASEPOINT, b))) for q, a, b in zip(dec, kt, ks)]
    cases.append(Case("ris_lincomb", [enc, rows(kt).reshape(n, 1, 5), rows(ks)], [enc_rows(want), flags([1] * n)], ok=1))
    return cases


def build_recoding_tile():
    spec = importlib.util.spec_from_file_location("sm_schedule_model", os.path.join(ROOT, "tools", "sm_schedule_model.py"))
    model = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(model)
    rng = random.Random(SEED + 110)
    ks = recoding_scalars()
    ks = ks + [rng.getrandbits(1 + (9 * j) % 252) | 1 for j in range(64 - len(ks))] + [rng.getrandbits(252) for _ in range(64 + 6)]
    pts = _recoding_points(len(ks), SEED + 111)
    want_steps = []
    for t in range(0, len(ks), 64):
        g, d, _ = model.tile_steps(ks[t:t + 64], depth=1)
        want_steps.append([g, d, 1])
    strict = pt_rows([pm.ed_scalar_mul(q, k) for q, k in zip(pts, ks)])
    cases = [Case("sm_tiles", [pt_rows(pts), rows(ks)], [strict, np.array(want_steps, dtype=np.int32)], rowwise=False, steps=True),
             Case("sm_tiles", [pt_rows(pts), rows(ks)], [strict])]
    # one tile each with a row off the curve (T Z = X Y holds) and a row with T Z = -X Y (on the curve): the gate must refuse both
    for kind in (0, 1):
        bad = list(pts[:64])
        x, y = rng.randrange(P), rng.randrange(P)
        g = bad[9]
        bad[9] = (x, y, 1, x * y % P) if kind == 0 else (g[0], g[1], g[2], (-g[3]) % P)
        k64 = [rng.getrandbits(40) | 1 << 39 for _ in range(64)]
        g = model.tile_steps(k64, depth=1, d_steps=False)[0]
        want = pt_rows([pm.ed_scalar_mul(q, k) for q, k in zip(bad, k64)])
        cases += [Case("sm_tiles", [pt_rows(bad), rows(k64)], [want, np.array([[g, 0, 0]], dtype=np.int32)], rowwise=False, steps=True),
                  Case("sm_tiles", [pt_rows(bad), rows(k64)], [want])]
    return cases


FAMILIES = {
    "field_core": Family("arith", build_field_core, "products, halves, powers, inverses, symbols and square roots on edge and random operands, both moduli"),
    "group_core": Family("arith", build_group_core, "the group law, the four scalar multiplications, codecs, equalities and validity on ordinary and junk points"),
    "sign_boundaries": Family("arith", build_sign_boundaries, "0, 1, (p-1)/2, (p+1)/2, p-1 through is_positive, |x|, the root's sign and both codecs"),
    "degenerate_encodings": Family("arith", build_degenerate_encodings, "s = 0, s = 1, t negative, non-squares; x = 0 with the sign bit, y = +-1"),
    "zero_by_value_p": Family("arith", build_zero_by_value_p, "k p and its non-zero neighbours through invert / div / to_affine, every launch form"),
    "zero_by_value_l": Family("scalar_ext", build_zero_by_value_l, "k L and its non-zero neighbours through sc_invert, every launch form"),
    "longest_inversions_p": Family("arith", build_longest_inversions_p, "the inputs of tests/golden/divsteps_worst.json mod p, every launch form and as Z"),
    "longest_inversions_l": Family("scalar_ext", build_longest_inversions_l, "the inputs of tests/golden/divsteps_worst.json mod L through sc_invert"),
    "scalar_ext": Family("scalar_ext", build_scalar_ext, "wide reduction and a b + c on edge and random operands"),
    "recoding_fast": Family("arith", build_recoding_fast, "recoding-edge scalars through the strict loop, both left-to-right forms and the windowed form"),
    "recoding_lincomb": Family("lincomb", build_recoding_lincomb, "the radix-16 digits themselves and ed_lincomb of one to three terms on them"),
    "recoding_base": Family("ris_lincomb", build_recoding_base, "the radix-256 digits themselves, mul_base and ris_lincomb's base term on them"),
    "recoding_tile": Family("sm_tile", build_recoding_tile, "the strict tile loop: step counts, recoding-edge scalars, rows the doubling gate must refuse"),
}
