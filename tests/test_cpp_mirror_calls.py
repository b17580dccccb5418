"""CPU tier: every wrapper of the C++ mirror (dusk_zerocaf_amd/include/zerocaf.hpp) runs against a recording stand-in.

tests/cpp/mirror_standin.py generates a libzerocaf_hip.so that defines every symbol the installed headers declare, computes
nothing, logs every call (by-value arguments and the full contents of every input extent) and fills every output extent with a
pattern.  tests/cpp/mirror_calls.cpp calls every function of zerocaf.hpp with inputs made by a formula and prints what each
returned.  Everything expected below -- the sequence of symbols per wrapper, every by-value argument, every input buffer byte
for byte, every returned object -- is computed here from that formula, from SHAPES (the extents, written from the headers'
documentation) and from the headers' row layout; nothing is recorded from a run of the wrappers.  Defects planted in copies of
the header must fail the comparison on the wrapper they touch and on no other.  g++ only; nothing is written inside the tree."""
import concurrent.futures
import importlib.util
import itertools
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

import pytest

from tests.entry_table import prototypes

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INC = os.path.join(ROOT, "include")
HPP = os.path.join(ROOT, "dusk_zerocaf_amd", "include", "zerocaf.hpp")
DRIVER = os.path.join(HERE, "cpp", "mirror_calls.cpp")

_spec = importlib.util.spec_from_file_location("mirror_standin", os.path.join(HERE, "cpp", "mirror_standin.py"))
SI = importlib.util.module_from_spec(_spec)
_bytecode, sys.dont_write_bytecode = sys.dont_write_bytecode, True           # no __pycache__ beside the generator: nothing is written in the tree
try:
    _spec.loader.exec_module(SI)
finally:
    sys.dont_write_bytecode = _bytecode
IN, OUT, MASK, IDOUT, PARTS, VALPTR, CTXOUT = SI.IN, SI.OUT, SI.MASK, SI.IDOUT, SI.PARTS, SI.VALPTR, SI.CTXOUT

HEADERS = ["zerocaf_hip.h"] + sorted(f for f in os.listdir(INC) if f.startswith("zerocaf_hip_ext"))


def all_prototypes(extra=""):
    protos = []
    for h in HEADERS:
        protos += prototypes(open(os.path.join(INC, h)).read())
    return protos + prototypes(extra)


# ---------------------------------------------------------------- the extents, from the headers' documentation
# Per symbol and pointer argument: inputs IN(element bytes, element count), outputs OUT(element bytes, elements per row, rows),
# accept masks MASK(rows); counts are expressions in the by-value arguments of the prototype.  FieldElement / Scalar: 5 words,
# EdwardsPoint: 20, ProjectivePoint: 15, affine: 10, encodings: 32 bytes (zerocaf_hip.h, "Data layout").
def _rows(width, size=8):
    return IN(size, "%d * n" % width)


L5, L15, L20, E32, E64 = _rows(5), _rows(15), _rows(20), _rows(32, 1), _rows(64, 1)
O5, O10, O15, O20, O80, O32, FLAG = OUT(8, 5), OUT(8, 10), OUT(8, 15), OUT(8, 20), OUT(8, 80), OUT(1, 32), OUT(1, 1)
ONE20 = OUT(8, 20, "1")
TERMS20, TERMS5, TERMS32 = IN(8, "20 * n * terms"), IN(8, "5 * n * terms"), IN(1, "32 * n * terms")
_HASH = dict(prefix=IN(1, "prefix_len"), parts=PARTS, part_len=IN(8, "nparts"))

SHAPES = {
    "zc_ctx_create": dict(devices=IN(4, "ndev"), out=CTXOUT),
    "zc_ctx_set_stream": dict(hip_stream=VALPTR),
    "zc_ctx_set_stream_dev": dict(hip_stream=VALPTR),
    "zc_host_register": dict(ptr=VALPTR),
    "zc_host_unregister": dict(ptr=VALPTR),
    "zc_fe_invert": dict(a=L5, out=O5, ok=MASK()),
    "zc_fe_div": dict(a=L5, b=L5, out=O5, ok=MASK()),
    "zc_fe_pow": dict(a=L5, e=L5, out=O5),
    "zc_fe_legendre_symbol": dict(a=L5, out=FLAG),
    "zc_fe_is_positive": dict(a=L5, out=FLAG),
    "zc_fe_mod_sqrt": dict(a=L5, out=O5, ok=MASK()),
    "zc_fe_from_bytes": dict(in32=E32, out=O5),
    "zc_fe_to_bytes": {"in": L5, "out32": O32},
    "zc_fe_sqrt_ratio_i": dict(u=L5, v=L5, out=O5, was_square=MASK()),
    "zc_fe_inv_sqrt": dict(a=L5, out=O5, was_square=MASK()),
    "zc_sc_pow": dict(a=L5, e=L5, out=O5),
    "zc_sc_from_bytes": dict(in32=E32, out=O5, ok=MASK()),
    "zc_sc_to_bytes": {"in": L5, "out32": O32},
    "zc_sc_shr": dict(a=L5, out=O5),
    "zc_sc_into_bits": dict(a=L5, bits256=OUT(1, 256)),
    "zc_sc_compute_naf": dict(a=L5, naf256=OUT(1, 256)),
    "zc_sc_from_bytes_wide": dict(in64=E64, out=O5),
    "zc_sc_from_bytes_mod_order": dict(in32=E32, out=O5),
    "zc_sc_muladd": dict(a=L5, b=L5, c=L5, out=O5),
    "zc_sc_invert": dict(a=L5, out=O5, ok=MASK()),
    "zc_ed_add": dict(p=L20, q=L20, out=O20),
    "zc_ed_sub": dict(p=L20, q=L20, out=O20),
    "zc_ed_double": dict(p=L20, out=O20),
    "zc_ed_neg": dict(p=L20, out=O20),
    "zc_ed_scalar_mul": dict(p=L20, k=L5, out=O20),
    "zc_ed_mul_by_pow_2": dict(p=L20, out=O20),
    "zc_ed_mul_by_cofactor": dict(p=L20, out=O20),
    "zc_ed_to_affine": dict(p=L20, xy_out=O10, ok=MASK()),
    "zc_ed_eq": dict(p=L20, q=L20, eq_out=FLAG),
    "zc_ed_compress": dict(p=L20, out32=O32, ok=MASK()),
    "zc_ed_decompress": dict(in32=E32, out=O20, ok=MASK()),
    "zc_ris_compress": dict(p=L20, out32=O32),
    "zc_ris_decompress": dict(in32=E32, out=O20, ok=MASK()),
    "zc_ris_eq": dict(p=L20, q=L20, eq_out=FLAG),
    "zc_ris_roundtrip_mul": dict(in32=E32, k=L5, out32=O32, ok=MASK()),
    "zc_ed_is_valid": dict(p=L20, valid_out=FLAG),
    "zc_ris_is_valid": dict(p=L20, valid_out=FLAG),
    "zc_ris_elligator": dict(r0=L5, out=O20),
    "zc_ris_from_uniform_bytes": dict(in64=E64, out=O20),
    "zc_proj_add": dict(p=L15, q=L15, out=O15),
    "zc_proj_sub": dict(p=L15, q=L15, out=O15),
    "zc_proj_double": dict(p=L15, out=O15),
    "zc_proj_neg": dict(p=L15, out=O15),
    "zc_proj_to_extended": dict(p=L15, out=O20),
    "zc_proj_eq": dict(p=L15, q=L15, eq=FLAG),
    "zc_proj_is_valid": dict(p=L15, valid=FLAG),
    "zc_proj_scalar_mul": dict(p=L15, k=L5, out=O15),
    "zc_ed_coset4": dict(p=L20, out4=O80),
    "zc_ed_mul_base": dict(k=L5, out=O20),
    "zc_ris_mul_base_compress": dict(k=L5, out32=O32),
    "zc_ed_mul_base_wnaf": dict(k=L5, out=O20),
    "zc_msm": dict(points=L20, scalars=L5, out_point=ONE20),
    "zc_msm_partial": dict(points=L20, scalars=L5, out_dev_point=ONE20),
    "zc_msm_plan": dict(out=OUT(4, 1, "nout < 17 ? nout : 17")),
    "zc_ed_fold_ordered": dict(parts=IN(8, "20 * count"), out=ONE20),
    "zc_comm_unique_id": dict(id_out128=OUT(1, 128, "1")),
    "zc_comm_init": dict(id128=IN(1, "128")),
    "zc_comm_size": dict(ranks=OUT(4, 1, "1")),
    "zc_msm_sharded": dict(points=IN(8, "20 * n_local"), scalars=IN(8, "5 * n_local"), out_point=ONE20),
    "zc_msm_bases_create": dict(points=L20, id_out=IDOUT("n")),
    "zc_msm_fixed": dict(scalars=IN(8, "5 * batch * TAB(id)"), out_points=OUT(8, 20, "batch")),
    "zc_msm_fixed_plan": dict(out=OUT(4, 1, "nout < 8 ? nout : 8")),
    "zc_msm_batch": dict(points=IN(8, "20 * n * batch"), scalars=IN(8, "5 * n * batch"), out_points=OUT(8, 20, "batch")),
    "zc_msm_batch_plan": dict(out=OUT(4, 1, "nout < 8 ? nout : 8")),
    "zc_ed_lincomb": dict(points=TERMS20, scalars=TERMS5, out=O20),
    "zc_ris_lincomb": dict(in32=TERMS32, scalars=TERMS5, base_scalars=L5, out32=O32, ok=MASK()),
    "zc_ris_double_and_compress": dict(p=L20, out32=O32),
    "zc_ris_lincomb_sum": dict(in32=TERMS32, scalars=TERMS5, base_scalars=L5, weights=L5, out32=OUT(1, 32, "1"), ok=MASK()),
    "zc_sha512_rows": dict(_HASH, out64=OUT(1, 64)),
    "zc_sc_from_sha512": dict(_HASH, out=O5),
    "zc_ris_from_sha512": dict(_HASH, out=O20),
    "zc_ed_scalar_mul_shared": dict(p=L20, k=IN(8, "5"), out=O20),
    "zc_ris_mul_shared": dict(in32=E32, k=IN(8, "5"), out32=O32, ok=MASK()),
    "zc_ed_lincomb_shared": dict(points=TERMS20, k=IN(8, "5 * terms"), out=O20),
    "zc_ris_lincomb_shared": dict(in32=TERMS32, k=IN(8, "5 * terms"), out32=O32, ok=MASK()),
    "zc_gens_create": dict(points=IN(8, "20 * count"), id_out=IDOUT("count")),
    "zc_ed_mul_gens": dict(scalars=IN(8, "5 * n * TAB(id)"), out=O20),
    "zc_ris_mul_gens_compress": dict(scalars=IN(8, "5 * n * TAB(id)"), out32=O32),
    "zc_ed_sum_rows": dict(points=TERMS20, out=O20),
    "zc_ris_sum_rows": dict(in32=TERMS32, out32=O32, ok=MASK()),
}
for _f in ("fe", "sc"):
    for _op in ("add", "sub", "mul"):
        SHAPES["zc_%s_%s" % (_f, _op)] = dict(a=L5, b=L5, out=O5)
    for _op in ("neg", "square", "half"):
        SHAPES["zc_%s_%s" % (_f, _op)] = dict(a=L5, out=O5)

PROTOS = all_prototypes()
ARGS = {name: SI.parse_args(text) for name, text in PROTOS}
SID = {name: i + 1 for i, name in enumerate(sorted(ARGS))}
# the symbols whose status the mirror hands to Backend::check (the others return a value, a string, or are called from destructors)
UNCHECKED = {"zc_ctx_destroy", "zc_msm_bases_destroy", "zc_gens_destroy", "zc_last_error", "zc_version", "zc_device_count", "zc_ctx_device_count"}


def has_ctx(sym):
    return any(t.replace("const", "").replace(" ", "") == "zc_ctx*" for t, _, _ in ARGS[sym])


def out_index(sym, arg):
    outs = [a for _, a, p in ARGS[sym] if p and SHAPES.get(sym, {}).get(a, ("",))[0] in ("out", "mask", "idout", "ctxout")]
    return outs.index(arg)


def pat(sym, arg, rows):
    """what the stand-in leaves in `rows` rows of output `arg` of `sym`"""
    s = SHAPES[sym][arg]
    if s[0] == "mask":
        return bytes(SI.mask_pattern(i) for i in range(rows))
    size, per, o = s[1], s[2], out_index(sym, arg)
    fmt = {8: "<Q", 4: "<i", 1: "<B"}[size]
    return b"".join(struct.pack(fmt, SI.pattern(SID[sym], o, i, w, size)) for i in range(rows) for w in range(per))


# ---------------------------------------------------------------- the driver's input formula (tests/cpp/mirror_calls.cpp)
def limbs(a, i=0, j=0, w0=0, count=5):
    return b"".join(struct.pack("<Q", (a << 40) | (i << 24) | (j << 8) | (w0 + w)) for w in range(count))


def sc(a, i=0, j=0):
    return limbs(a, i, j)


def pt(a, i=0, j=0):
    return limbs(a, i, j, 0, 20)


def pj(a):
    return limbs(a, 0, 0, 0, 15)


def by(a, i=0, j=0, n=32):
    return bytes([a, i, j][b] if b < 3 else (13 * b + a + i + j) & 255 for b in range(n))


def cat(f, a, n, t=None):
    """row-major: row i owns its t consecutive elements"""
    if t is None:
        return b"".join(f(a, i) for i in range(n))
    return b"".join(f(a, i, j) for i in range(n) for j in range(t))


PTR, NULL = "PTR", "NULL"
ANY_PTR = ("PTR", "NULL")                   # an output nobody writes (no rows): null or not
ANY_ORDER = "any order"                     # (ANY_ORDER, [records]): the records of a segment whose order the language leaves open
NONE_TO_READ = ("", "NULL")               # an input of no elements where the header takes either


def call(sym, **args):
    """an expected record: bytes -> their hexadecimal text, integers -> decimal; a tuple lists the values that are all right"""
    want = {"ctx": "ok"} if has_ctx(sym) else {}
    for k, v in args.items():
        k = k.rstrip("_").replace("__", ".")
        want[k] = v.hex() if isinstance(v, bytes) else str(v) if isinstance(v, int) else v
    return (sym, want)


class Ids:
    """the ids the stand-in hands out: one counter for both kinds of table, in the order of the create calls"""

    def __init__(self):
        self.next = SI.FIRST_ID

    def take(self):
        self.next += 1
        return self.next - 1


def point_at(blob, i):
    return blob[160 * i:160 * (i + 1)]


# ---------------------------------------------------------------- single-element operators: one symbol, rows of one
def single(sym, ins, rets, **vals):
    """ins: [(argument, bytes)]; rets: [(printed name, 'out' / 'bool' / 'mask', argument)]"""
    def build(p, ids):
        args = dict(ins)
        args.update(vals)
        for _, a, is_ptr in ARGS[sym]:
            if is_ptr and SHAPES.get(sym, {}).get(a, ("",))[0] in ("out", "mask"):
                args[a] = PTR
        if any(a == "n" for _, a, _ in ARGS[sym]):
            args["n"] = 1
        printed = []
        for name, how, a in rets:
            v = pat(sym, a, 1)
            printed.append((name, v.hex() if how == "out" else "01" if any(v) else "00"))
        return [call(sym, **args)], printed
    return build


def twice(sym, arg, out):
    """operator== of FieldElement / Scalar: both operands through to_bytes (C++ leaves the order of the two to the compiler),
    equal patterns compare equal"""
    def build(p, ids):
        return (ANY_ORDER, [call(sym, **{arg: limbs(1), out: PTR, "n": 1}), call(sym, **{arg: limbs(2), out: PTR, "n": 1})]), [("ret", "01")]
    return build


F1, F2, S3 = limbs(1), limbs(2), limbs(3)
R_OUT = [("ret", "out", "out")]
EXPECT = {
    "Backend::ctx": lambda p, ids: ([call("zc_ctx_create", devices=NULL, ndev=0, out=PTR)], [("nonnull", "01")]),
    "Backend::check": lambda p, ids: ([call("zc_last_error")], "runtime_error probe failed: " + SI.LAST_ERROR),
    "Backend::device_count": lambda p, ids: ([call("zc_device_count")], [("ret", "3")]),
    "Backend::version": lambda p, ids: ([call("zc_version")], [("ret", SI.VERSION.encode().hex())]),
    "Backend::set_stream": lambda p, ids: ([call("zc_ctx_set_stream", hip_stream="0x1230", external=1)], []),
    "Backend::use_own_stream": lambda p, ids: ([call("zc_ctx_set_stream", hip_stream="0x0", external=0)], []),
    "Backend::synchronize": lambda p, ids: ([call("zc_ctx_synchronize")], []),
    "Backend::device": lambda p, ids: ([call("zc_ctx_device", slot=2)], [("ret", "1")]),
    "Backend::slot_count": lambda p, ids: ([call("zc_ctx_device_count")], [("ret", "2")]),
    "Backend::set_stream_dev": lambda p, ids: ([call("zc_ctx_set_stream_dev", slot=3, hip_stream="0x4560", external=1)], []),
    "Backend::host_register": lambda p, ids: ([call("zc_host_register", ptr="0x7890", bytes=4096)], []),
    "Backend::host_unregister": lambda p, ids: ([call("zc_host_unregister", ptr="0x7890")], []),
    "Backend::comm_unique_id": lambda p, ids: ([call("zc_comm_unique_id", id_out128=PTR)], [("ret", pat("zc_comm_unique_id", "id_out128", 1).hex())]),
    "Backend::comm_init": lambda p, ids: ([call("zc_comm_init", id128=by(1, n=128), rank=2, world=5)], []),
    "Backend::comm_size": lambda p, ids: ([call("zc_comm_size", ranks=PTR)], [("ret", str(struct.unpack("<i", pat("zc_comm_size", "ranks", 1))[0]))]),
    "Backend::comm_destroy": lambda p, ids: ([call("zc_comm_destroy")], []),
    "exit": lambda p, ids: ([call("zc_ctx_destroy")], []),
    "FieldElement::operator+": single("zc_fe_add", [("a", F1), ("b", F2)], R_OUT),
    "FieldElement::operator-": single("zc_fe_sub", [("a", F1), ("b", F2)], R_OUT),
    "FieldElement::operator*": single("zc_fe_mul", [("a", F1), ("b", F2)], R_OUT),
    "FieldElement::neg": single("zc_fe_neg", [("a", F1)], R_OUT),
    "FieldElement::square": single("zc_fe_square", [("a", F1)], R_OUT),
    "FieldElement::inverse": single("zc_fe_invert", [("a", F1)], R_OUT),
    "FieldElement::operator/": single("zc_fe_div", [("a", F1), ("b", F2)], R_OUT),
    "FieldElement::half": single("zc_fe_half", [("a", F1)], R_OUT),
    "FieldElement::pow": single("zc_fe_pow", [("a", F1), ("e", F2)], R_OUT),
    "FieldElement::legendre_symbol": single("zc_fe_legendre_symbol", [("a", F1)], [("ret", "bool", "out")]),
    "FieldElement::is_positive": single("zc_fe_is_positive", [("a", F1)], [("ret", "bool", "out")]),
    "FieldElement::mod_sqrt": lambda p, ids: single("zc_fe_mod_sqrt", [("a", F1)], [("has", "mask", "ok")] + R_OUT, sign=p["sign"])(p, ids),
    "FieldElement::sqrt_ratio_i": single("zc_fe_sqrt_ratio_i", [("u", F1), ("v", F2)], [("first", "mask", "was_square"), ("second", "out", "out")]),
    "FieldElement::inv_sqrt": single("zc_fe_inv_sqrt", [("a", F1)], [("first", "mask", "was_square"), ("second", "out", "out")]),
    "FieldElement::from_bytes": single("zc_fe_from_bytes", [("in32", by(1))], R_OUT),
    "FieldElement::to_bytes": single("zc_fe_to_bytes", [("in", F1)], [("ret", "out", "out32")]),
    "FieldElement::operator==": twice("zc_fe_to_bytes", "in", "out32"),
    "Scalar::operator+": single("zc_sc_add", [("a", F1), ("b", F2)], R_OUT),
    "Scalar::operator-": single("zc_sc_sub", [("a", F1), ("b", F2)], R_OUT),
    "Scalar::operator*": single("zc_sc_mul", [("a", F1), ("b", F2)], R_OUT),
    "Scalar::neg": single("zc_sc_neg", [("a", F1)], R_OUT),
    "Scalar::square": single("zc_sc_square", [("a", F1)], R_OUT),
    "Scalar::half": single("zc_sc_half", [("a", F1)], R_OUT),
    "Scalar::pow": single("zc_sc_pow", [("a", F1), ("e", F2)], R_OUT),
    "Scalar::operator>>": single("zc_sc_shr", [("a", F1)], R_OUT, shift=9),
    "Scalar::into_bits": single("zc_sc_into_bits", [("a", F1)], [("ret", "out", "bits256")]),
    "Scalar::compute_NAF": single("zc_sc_compute_naf", [("a", F1)], [("ret", "out", "naf256")], width=0),
    "Scalar::compute_window_NAF": single("zc_sc_compute_naf", [("a", F1)], [("ret", "out", "naf256")], width=5),
    "Scalar::from_bytes": single("zc_sc_from_bytes", [("in32", by(1))], R_OUT),
    "Scalar::from_bytes_wide": single("zc_sc_from_bytes_wide", [("in64", by(1, n=64))], R_OUT),
    "Scalar::from_bytes_mod_order": single("zc_sc_from_bytes_mod_order", [("in32", by(1))], R_OUT),
    "Scalar::muladd": single("zc_sc_muladd", [("a", F1), ("b", F2), ("c", S3)], R_OUT),
    "Scalar::invert": single("zc_sc_invert", [("a", F1)], R_OUT),
    "Scalar::to_bytes": single("zc_sc_to_bytes", [("in", F1)], [("ret", "out", "out32")]),
    "Scalar::operator==": twice("zc_sc_to_bytes", "in", "out32"),
    "EdwardsPoint::operator+": single("zc_ed_add", [("p", pt(1)), ("q", pt(2))], R_OUT),
    "EdwardsPoint::operator-": single("zc_ed_sub", [("p", pt(1)), ("q", pt(2))], R_OUT),
    "EdwardsPoint::neg": single("zc_ed_neg", [("p", pt(1))], R_OUT),
    "EdwardsPoint::double_": single("zc_ed_double", [("p", pt(1))], R_OUT),
    "EdwardsPoint::operator*": single("zc_ed_scalar_mul", [("p", pt(1)), ("k", F2)], R_OUT, flags=0),
    "EdwardsPoint::operator==": single("zc_ed_eq", [("p", pt(1)), ("q", pt(2))], [("ret", "bool", "eq_out")]),
    "EdwardsPoint::is_valid": single("zc_ed_is_valid", [("p", pt(1))], [("ret", "bool", "valid_out")]),
    "EdwardsPoint::compress": single("zc_ed_compress", [("p", pt(1))], [("ret", "out", "out32")]),
    "AffinePoint::from": lambda p, ids: (single("zc_ed_to_affine", [("p", pt(1))], [])(p, ids)[0],
                                         [("X", pat("zc_ed_to_affine", "xy_out", 1)[:40].hex()), ("Y", pat("zc_ed_to_affine", "xy_out", 1)[40:].hex())]),
    "ProjectivePoint::operator+": single("zc_proj_add", [("p", pj(1)), ("q", pj(2))], R_OUT),
    "ProjectivePoint::double_": single("zc_proj_double", [("p", pj(1))], R_OUT),
    "ProjectivePoint::to_extended": single("zc_proj_to_extended", [("p", pj(1))], R_OUT),
    "ProjectivePoint::neg": single("zc_proj_neg", [("p", pj(1))], R_OUT),
    "ProjectivePoint::operator-": single("zc_proj_sub", [("p", pj(1)), ("q", pj(2))], R_OUT),
    "ProjectivePoint::operator*": single("zc_proj_scalar_mul", [("p", pj(1)), ("k", F2)], R_OUT),
    "ProjectivePoint::operator==": single("zc_proj_eq", [("p", pj(1)), ("q", pj(2))], [("ret", "bool", "eq")]),
    "ProjectivePoint::is_valid": single("zc_proj_is_valid", [("p", pj(1))], [("ret", "bool", "valid")]),
    "coset4": single("zc_ed_coset4", [("p", pt(1))], [("ret", "out", "out4")]),
    "CompressedEdwardsY::decompress": single("zc_ed_decompress", [("in32", by(1))], [("has", "mask", "ok")] + R_OUT),
    "mul_by_pow_2": single("zc_ed_mul_by_pow_2", [("p", pt(1))], R_OUT, kexp=77),
    "mul_by_cofactor": single("zc_ed_mul_by_cofactor", [("p", pt(1))], R_OUT),
    "RistrettoPoint::operator==": single("zc_ris_eq", [("p", pt(1)), ("q", pt(2))], [("ret", "bool", "eq_out")]),
    "RistrettoPoint::is_valid": single("zc_ris_is_valid", [("p", pt(1))], [("ret", "bool", "valid_out")]),
    "RistrettoPoint::elligator_ristretto_flavor": single("zc_ris_elligator", [("r0", F1)], R_OUT),
    "RistrettoPoint::from_uniform_bytes": single("zc_ris_from_uniform_bytes", [("in64", by(1, n=64))], R_OUT),
    "RistrettoPoint::compress": single("zc_ris_compress", [("p", pt(1))], [("ret", "out", "out32")]),
    "CompressedRistretto::decompress": single("zc_ris_decompress", [("in32", by(1))], [("has", "mask", "ok")] + R_OUT),
}


def expect(name):
    def deco(fn):
        EXPECT[name] = fn
        return fn
    return deco


# ---------------------------------------------------------------- the wrappers that pack rows
def rowwise(name, sym, ins, outs, **vals):
    """A wrapper over one batched symbol: no rows, no call; ins [(argument, bytes of n rows)], outs [(printed, argument)]"""
    @expect(name)
    def build(p, ids):
        n = p["n"]
        if n == 0:
            return [], [(printed, "") for printed, _ in outs]
        args = {a: f(n) for a, f in ins}
        args.update({a: PTR for _, a in outs})
        args.update(vals)
        return [call(sym, n=n, **args)], [(printed, pat(sym, a, n).hex()) for printed, a in outs]


rowwise("mul_batch", "zc_ed_scalar_mul", [("p", lambda n: cat(pt, 1, n)), ("k", lambda n: cat(sc, 2, n))], [("ret", "out")], flags=0)
rowwise("mul_batch_fe", "zc_fe_mul", [("a", lambda n: cat(sc, 1, n)), ("b", lambda n: cat(sc, 2, n))], [("ret", "out")])
rowwise("double_and_compress_batch", "zc_ris_double_and_compress", [("p", lambda n: cat(pt, 1, n))], [("ret", "out32")])
rowwise("mul_base_batch", "zc_ed_mul_base", [("k", lambda n: cat(sc, 1, n))], [("ret", "out")])
rowwise("window_naf_mul_batch", "zc_ed_mul_base_wnaf", [("k", lambda n: cat(sc, 1, n))], [("ret", "out")], width=6)
rowwise("ristretto_keygen_batch", "zc_ris_mul_base_compress", [("k", lambda n: cat(sc, 1, n))], [("ret", "out32")])
rowwise("scalar_mul_shared", "zc_ed_scalar_mul_shared", [("p", lambda n: cat(pt, 1, n)), ("k", lambda n: sc(2))], [("ret", "out")])
rowwise("ris_mul_shared", "zc_ris_mul_shared", [("in32", lambda n: cat(by, 1, n)), ("k", lambda n: sc(2))], [("ret", "out32"), ("ok", "ok")])


@expect("ristretto_roundtrip_mul_batch")
def _(p, ids):
    n = p["n"]
    if n == 0:
        return [], [("has", ""), ("ret", "")]
    sym = "zc_ris_roundtrip_mul"
    out, ok = pat(sym, "out32", n), pat(sym, "ok", n)
    kept = b"".join(out[32 * i:32 * (i + 1)] for i in range(n) if ok[i])
    return [call(sym, in32=cat(by, 1, n), k=cat(sc, 2, n), out32=PTR, ok=PTR, n=n)], [("has", ok.hex()), ("ret", kept.hex())]


@expect("msm")
def _(p, ids):
    n = p["n"]            # no pairs: still a call (the empty sum is the library's), on pointers that are not null
    return [call("zc_msm", points=cat(pt, 1, n), scalars=cat(sc, 2, n), n=n, out_point=PTR)], [("ret", pat("zc_msm", "out_point", 1).hex())]


@expect("fold_ordered")
def _(p, ids):
    n = p["n"]
    return [call("zc_ed_fold_ordered", parts=cat(pt, 1, n), count=n, out=PTR)], [("ret", pat("zc_ed_fold_ordered", "out", 1).hex())]


@expect("msm_sharded")
def _(p, ids):
    n = p["n"]
    return ([call("zc_msm_sharded", points=cat(pt, 1, n) if n else NONE_TO_READ, scalars=cat(sc, 2, n) if n else NONE_TO_READ, n_local=n, out_point=PTR)],
            [("ret", pat("zc_msm_sharded", "out_point", 1).hex())])


@expect("msm_partial")
def _(p, ids):
    n = p["n"]
    return ([call("zc_msm_partial", points=cat(pt, 1, n), scalars=cat(sc, 2, n), n=n, out_dev_point=PTR)],
            [("out_dev", pat("zc_msm_partial", "out_dev_point", 1).hex())])


@expect("msm_plan")
def _(p, ids):
    return [call("zc_msm_plan", n=p["n"], points_aligned16=p["aligned"], out=PTR, nout=17)], [("ret", pat("zc_msm_plan", "out", 17).hex())]


@expect("msm_batch_plan")
def _(p, ids):
    return ([call("zc_msm_batch_plan", n=p["n"], batch=p["batch"], points_aligned16=p["aligned"], out=PTR, nout=8)],
            [("ret", pat("zc_msm_batch_plan", "out", 8).hex())])


@expect("MsmBases::plan")
def _(p, ids):
    return [call("zc_msm_fixed_plan", n=p["n"], window_bits=p["window_bits"], out=PTR, nout=8)], [("ret", pat("zc_msm_fixed_plan", "out", 8).hex())]


@expect("msm_batch")
def _(p, ids):
    if "variant" in p:
        return [], "invalid_argument"
    batch = p["batch"]
    n = p["n"] if batch else 0            # instance-major: instance b owns rows [b n, (b + 1) n)
    return ([call("zc_msm_batch", points=cat(pt, 1, batch, n), scalars=cat(sc, 2, batch, n), n=n, batch=batch, out_points=PTR if batch else ANY_PTR)],
            [("ret", pat("zc_msm_batch", "out_points", batch).hex())])


@expect("ed_lincomb")
def _(p, ids):
    if "variant" in p:
        return [], "invalid_argument"
    n, t = p["n"], p["t"]
    if n == 0:
        return [], [("ret", "")]
    return [call("zc_ed_lincomb", points=cat(pt, 1, n, t), scalars=cat(sc, 2, n, t), terms=t, out=PTR, n=n)], [("ret", pat("zc_ed_lincomb", "out", n).hex())]


@expect("ris_lincomb")
def _(p, ids):
    if "variant" in p:
        return [], "invalid_argument"
    n, t = p["n"], p["t"]
    if n == 0:
        return [], [("ret", ""), ("ok", "")]
    sym = "zc_ris_lincomb"
    return ([call(sym, in32=cat(by, 1, n, t), scalars=cat(sc, 2, n, t), terms=t, base_scalars=cat(sc, 3, n) if p["bs"] else NULL, out32=PTR, ok=PTR, n=n)],
            [("ret", pat(sym, "out32", n).hex()), ("ok", pat(sym, "ok", n).hex())])


@expect("ris_lincomb_sum")
def _(p, ids):
    if "variant" in p:
        return [], "invalid_argument"
    n, t = p["n"], p["t"]
    sym = "zc_ris_lincomb_sum"          # no rows: still a call (the empty sum), on pointers that are not null
    return ([call(sym, in32=cat(by, 1, n, t), scalars=cat(sc, 2, n, t), terms=t if n else 1, base_scalars=cat(sc, 3, n) if p["bs"] and n else NULL,
                  weights=cat(sc, 4, n) if p["zs"] and n else NULL, out32=PTR, ok=PTR if n else ANY_PTR, n=n)],
            [("ret", pat(sym, "out32", 1).hex()), ("ok", pat(sym, "ok", n).hex())])


def shared_lincomb(name, sym, elem, first, outs):
    @expect(name)
    def build(p, ids):
        if "variant" in p:
            return [], "invalid_argument"
        n, t = p["n"], p["t"]
        if n == 0:
            return [], [(printed, "") for printed, _ in outs]
        args = {first: cat(elem, 1, n, t), "k": cat(sc, 2, t), "terms": t, "n": n}
        args.update({a: PTR for _, a in outs})
        return [call(sym, **args)], [(printed, pat(sym, a, n).hex()) for printed, a in outs]


shared_lincomb("ed_lincomb_shared", "zc_ed_lincomb_shared", pt, "points", [("ret", "out")])
shared_lincomb("ris_lincomb_shared", "zc_ris_lincomb_shared", by, "in32", [("ret", "out32"), ("ok", "ok")])


@expect("MsmBases")
def _(p, ids):
    v, fixed = p["variant"], "zc_msm_fixed"

    def mk(a, n, wb=0):
        return ids.take(), call("zc_msm_bases_create", points=cat(pt, a, n), n=n, window_bits=wb, id_out=PTR)
    destroy = lambda i: call("zc_msm_bases_destroy", id=i)
    if v == "use":
        i, c = mk(1, 3, p["window_bits"])
        two = pat(fixed, "out_points", 2)
        return ([c, call(fixed, id=i, scalars=cat(sc, 2, 3), batch=1, out_points=PTR), call(fixed, id=i, scalars=cat(sc, 3, 2, 3), batch=2, out_points=PTR),
                 call(fixed, id=i, scalars=NONE_TO_READ, batch=0, out_points=ANY_PTR), destroy(i)],
                [("size", "3"), ("one", point_at(two, 0).hex()), ("two", two.hex()), ("none", "")])
    if v == "move":                     # the moved-from object destroys nothing: one destroy, with the id create produced
        i, c = mk(1, 3)
        return [c, call(fixed, id=i, scalars=cat(sc, 2, 3), batch=1, out_points=PTR), destroy(i)], [("moved", pat(fixed, "out_points", 1).hex())]
    if v == "move_assign":              # the overwritten table goes first
        i, c = mk(1, 3)
        j, d = mk(2, 2)
        return ([c, d, destroy(j), call(fixed, id=i, scalars=cat(sc, 3, 3), batch=1, out_points=PTR), destroy(i)],
                [("size", "3"), ("assigned", pat(fixed, "out_points", 1).hex())])
    assert v == "ragged"
    i, c = mk(1, 3)
    return [c, destroy(i)], "invalid_argument"


@expect("Generators")
def _(p, ids):
    v, mul, mulc = p["variant"], "zc_ed_mul_gens", "zc_ris_mul_gens_compress"

    def mk(a, count):
        i = ids.take()
        return i, call("zc_gens_create", points=cat(pt, a, count), count=count, id_out=PTR)
    destroy = lambda i: call("zc_gens_destroy", id=i)
    if v == "use":
        count = p["count"]
        i, c = mk(1, count)
        return ([c, call(mul, id=i, scalars=cat(sc, 2, 3, count), out=PTR, n=3), call(mulc, id=i, scalars=cat(sc, 3, 3, count), out32=PTR, n=3), destroy(i)],
                [("size", str(count)), ("mul", pat(mul, "out", 3).hex()), ("mul_compress", pat(mulc, "out32", 3).hex()), ("mul0", ""), ("mul_compress0", "")])
    if v == "move":
        i, c = mk(1, 2)
        return [c, call(mul, id=i, scalars=cat(sc, 2, 3, 2), out=PTR, n=3), destroy(i)], [("moved", pat(mul, "out", 3).hex())]
    if v == "move_assign":
        i, c = mk(1, 2)
        j, d = mk(2, 1)
        return ([c, d, destroy(j), call(mulc, id=i, scalars=cat(sc, 3, 3, 2), out32=PTR, n=3), destroy(i)],
                [("size", "2"), ("assigned", pat(mulc, "out32", 3).hex())])
    assert v in ("ragged", "wrong_length", "ragged_compress")
    i, c = mk(1, 3)
    return [c, destroy(i)], "invalid_argument"


@expect("sum_rows_ed")
def _(p, ids):
    if "variant" in p:
        return [], "invalid_argument"
    n, t = p["n"], p["t"]
    if n == 0:
        return [], [("ret", "")]
    return [call("zc_ed_sum_rows", points=cat(pt, 1, n, t), terms=t, out=PTR, n=n)], [("ret", pat("zc_ed_sum_rows", "out", n).hex())]


@expect("sum_rows_wire")
def _(p, ids):
    if "variant" in p:
        return [], "invalid_argument"
    n, t, sym = p["n"], p["t"], "zc_ris_sum_rows"
    took = [("ok", pat(sym, "ok", n).hex())] if p["ok"] else []           # the mask is passed through; not taking it is accepted
    if n == 0:
        return [], [("ret", "")] + took
    return [call(sym, in32=cat(by, 1, n, t), terms=t, out32=PTR, ok=PTR, n=n)], [("ret", pat(sym, "out32", n).hex())] + took


HASH_ROW_BYTES = (1, 5, 130, 32)


def hashing(name, sym, out):
    @expect(name)
    def build(p, ids):
        nparts, prefix = p["nparts"], b"\x01pq"[:p["prefix"]]
        args = {"prefix": prefix, "prefix_len": len(prefix), "part_len": struct.pack("<%dQ" % nparts, *HASH_ROW_BYTES[:nparts]), "nparts": nparts, out: PTR, "n": 3}
        for j in range(nparts):
            args["parts__%d" % j] = b"".join(by(1, i, j, HASH_ROW_BYTES[j]) for i in range(3))
        return [call(sym, **args)], [("out", pat(sym, out, 3).hex())]


hashing("sha512_rows", "zc_sha512_rows", "out64")
hashing("sc_from_sha512", "zc_sc_from_sha512", "out")
hashing("ris_from_sha512", "zc_ris_from_sha512", "out")
for _name in ("mul_batch", "mul_batch_fe", "ristretto_roundtrip_mul_batch", "msm"):
    EXPECT[_name] = (lambda inner: lambda p, ids: ([], "invalid_argument") if "variant" in p else inner(p, ids))(EXPECT[_name])


# ---------------------------------------------------------------- running the driver and comparing
def parse_label(label):
    toks = label.split()
    p = {}
    for tok in toks[1:]:
        if "=" in tok:
            k, v = tok.split("=")
            p[k] = int(v)
        else:
            p["variant"] = tok
    return toks[0], p


def segments(lines):
    """[(label, [lines])] from the lines between marks"""
    out = []
    for line in lines:
        if line.startswith("@ "):
            out.append((line[2:], []))
        elif line:
            assert out, "a line before the first mark: %r" % line
            out[-1][1].append(line)
    return out


def parse_record(line):
    toks = line.split(" ")
    rec = {}
    for tok in toks[1:]:
        k, _, v = tok.partition("=")
        assert k not in rec, line
        rec[k] = v
    return toks[0], rec


def matches(want, got):
    if want[0] != got[0] or set(want[1]) != set(got[1]):
        return False
    return all(got[1][k] in v if isinstance(v, tuple) else got[1][k] == v for k, v in want[1].items())


def describe(want, got):
    if want is None or got is None or want[0] != got[0]:
        return "call %s where %s was expected" % (got and got[0], want and want[0])
    bad = [k for k in sorted(set(want[1]) | set(got[1])) if k not in want[1] or k not in got[1] or not (got[1][k] in want[1][k] if isinstance(want[1][k], tuple) else got[1][k] == want[1][k])]
    return "%s: arguments %s differ" % (want[0], bad)


class Run:
    def __init__(self, returncode, stdout, stderr, log):
        self.returncode, self.stdout, self.stderr = returncode, stdout, stderr
        self.out = segments(stdout.splitlines())
        self.log = [(label, [parse_record(l) for l in lines]) for label, lines in segments(log.splitlines())]


def run_driver(exe, tmp, env=None):
    fd, log = tempfile.mkstemp(suffix=".log", dir=tmp)
    os.close(fd)
    full = dict(os.environ, ZC_STANDIN_LOG=log, **(env or {}))
    r = subprocess.run([exe], env=full, capture_output=True, text=True, timeout=120)
    return Run(r.returncode, r.stdout, r.stderr, open(log).read() if os.path.exists(log) else "")


def failures(run, returns=True):
    """['<label>: what differs'] -- the comparison of a whole run with the expectations above; returns=False: the calls only"""
    bad = []
    if run.returncode != 0:
        bad.append("driver: exit status %d: %s" % (run.returncode, run.stderr[-400:]))
    if [l for l, _ in run.out] != [l for l, _ in run.log]:
        bad.append("driver: the marks of the log and of the output differ")
        return bad
    ids = Ids()
    for (label, printed), (_, records) in zip(run.out, run.log):
        name, p = parse_label(label)
        if name not in EXPECT:
            bad.append("%s: no expectation for this wrapper" % label)
            continue
        calls, rets = EXPECT[name](p, ids)
        if isinstance(calls, tuple) and calls[0] == ANY_ORDER:
            calls = next((list(c) for c in itertools.permutations(calls[1]) if len(c) == len(records) and all(matches(w, g) for w, g in zip(c, records))), calls[1])
        if len(calls) != len(records) or not all(matches(w, g) for w, g in zip(calls, records)):
            n = min(len(calls), len(records))
            first = next((i for i in range(n) if not matches(calls[i], records[i])), n)
            bad.append("%s: call %d: %s (%d calls, %d expected)" % (label, first, describe(calls[first] if first < len(calls) else None,
                                                                                           records[first] if first < len(records) else None), len(records), len(calls)))
            continue
        if isinstance(rets, str):               # the exception the wrapper must leave with, and the start of its message
            if len(printed) != 1 or not (printed[0] + " ").startswith("! %s " % rets):
                bad.append("%s: std::%s expected, got %r" % (label, rets, [l[:60] for l in printed]))
        elif returns:
            want = ["= %s %s" % (k, v) if v else "= %s " % k for k, v in rets]
            if want != printed:
                which = [k for (k, _), w, g in zip(rets, want, printed + [None] * len(want)) if w != g]
                bad.append("%s: returned %s differ%s" % (label, which, "" if len(want) == len(printed) else " (%d lines, %d expected)" % (len(printed), len(want))))
    return bad


# ---------------------------------------------------------------- building
def copy_tree(where, edits=()):
    """the headers as a checkout has them; edits: [(old, new)] applied to the copy of zerocaf.hpp, each old exactly once"""
    os.makedirs(os.path.join(where, "include"))
    os.makedirs(os.path.join(where, "dusk_zerocaf_amd", "include"))
    for h in HEADERS:
        shutil.copy(os.path.join(INC, h), os.path.join(where, "include"))
    text = open(HPP).read()
    for old, new in edits:
        assert text.count(old) == 1, old
        text = text.replace(old, new)
    with open(os.path.join(where, "dusk_zerocaf_amd", "include", "zerocaf.hpp"), "w") as f:
        f.write(text)
    return os.path.join(where, "dusk_zerocaf_amd", "include")


SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def build_standin(where, flags=(), extra_header=""):
    os.makedirs(where, exist_ok=True)
    src = os.path.join(where, "standin.cpp")
    with open(src, "w") as f:
        f.write(SI.source(all_prototypes(extra_header), SHAPES))
    so = os.path.join(where, "libzerocaf_hip.so")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-fPIC", "-shared", "-Wall", *flags, "-I" + INC, "-o", so, src])
    return so


def build_driver(where, libdir, edits=(), flags=()):
    inc = copy_tree(os.path.join(where, "tree"), edits)
    exe = os.path.join(where, "mirror_calls")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-Wall", "-Wextra", "-Werror", *flags, "-I" + inc, DRIVER, "-o", exe, "-L" + libdir, "-lzerocaf_hip", "-Wl,-rpath," + libdir])
    return exe


def sanitizers_link(tmp):
    src = os.path.join(tmp, "probe.cpp")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    return subprocess.run(["g++", *SAN, src, "-o", os.path.join(tmp, "probe")], capture_output=True).returncode == 0


# One defect per copy of the header.  wrappers: where the comparison must fail, and nowhere else; cases / spared_cases: segments
# that must (not) be among the failures.  calls_only: the defect makes the library write more rows than the wrapper allocated, so
# the stand-in runs with ZC_STANDIN_NOFILL and only the logged calls are compared.
MUTANTS = [
    dict(name="ed_lincomb_term_major", wrappers={"ed_lincomb"}, cases=["ed_lincomb n=3 t=2", "ed_lincomb n=3 t=8"], spared_cases=["ed_lincomb n=3 t=1", "ed_lincomb n=1 t=8"],
         edits=[("        for (size_t j = 0; j < t; j++) {\n            pss[i][j].flat(&p[20 * (i * t + j)]);", "        for (size_t j = 0; j < t; j++) {\n            pss[i][j].flat(&p[20 * (j * n + i)]);")]),
    dict(name="ris_lincomb_sum_b_and_z_exchanged", wrappers={"ris_lincomb_sum"}, cases=["ris_lincomb_sum n=3 t=2 bs=1 zs=0", "ris_lincomb_sum n=1 t=1 bs=1 zs=1"],
         spared_cases=["ris_lincomb_sum n=3 t=2 bs=0 zs=0"],
         edits=[("bs.empty() ? nullptr : b.data(), zs.empty() ? nullptr : z.data(), o, ok.data(), n)", "zs.empty() ? nullptr : z.data(), bs.empty() ? nullptr : b.data(), o, ok.data(), n)")]),
    # (an empty std::vector's data() is null anyway: the defect passes a zeroed array of base scalars where none was given)
    dict(name="ris_lincomb_bs_passed_when_empty", wrappers={"ris_lincomb"}, cases=["ris_lincomb n=3 t=2 bs=0"], spared_cases=["ris_lincomb n=3 t=2 bs=1"],
         edits=[("k(n * t * 5), b(bs.size() * 5);", "k(n * t * 5), b(n * 5);"), ("t, bs.empty() ? nullptr : b.data(), o.data(), ok.data(), n), \"zc_ris_lincomb\")", "t, b.data(), o.data(), ok.data(), n), \"zc_ris_lincomb\")")]),
    dict(name="msm_batch_n_and_batch_exchanged", wrappers={"msm_batch"}, cases=["msm_batch batch=2 n=3"], calls_only=True,
         edits=[("k.data(), n, batch, o.data()), \"zc_msm_batch\")", "k.data(), batch, n, o.data()), \"zc_msm_batch\")")]),
    dict(name="msm_fixed_stride_of_the_batch", wrappers={"MsmBases"}, cases=["MsmBases use window_bits=0", "MsmBases use window_bits=9"], spared_cases=["MsmBases move"],
         edits=[("std::memcpy(&k[5 * (b * n_ + i)], kss[b][i].l.data(), 40);", "std::memcpy(&k[5 * (b * kss.size() + i)], kss[b][i].l.data(), 40);")]),
    dict(name="gens_row_length_of_the_first_row", wrappers={"Generators"}, cases=["Generators wrong_length"], spared_cases=["Generators use count=2"],
         edits=[("if (kss[i].size() != count_) throw", "if (kss[i].size() != kss[0].size()) throw")]),
    dict(name="ris_mul_shared_rows_reversed", wrappers={"ris_mul_shared"}, cases=["ris_mul_shared n=3"], spared_cases=["ris_mul_shared n=1"],
         edits=[("\"zc_ris_mul_shared\");\n    for (size_t i = 0; i < n; i++) std::memcpy(out[i].bytes.data(), &o[32 * i], 32);",
                 "\"zc_ris_mul_shared\");\n    for (size_t i = 0; i < n; i++) std::memcpy(out[i].bytes.data(), &o[32 * (n - 1 - i)], 32);")]),
    # (the first part has rows of one byte, so the defect stays inside the arrays: it hashes one part where four were given)
    dict(name="sha512_rows_nparts_from_the_first_length", wrappers={"sha512_rows"}, cases=["sha512_rows nparts=4 prefix=0", "sha512_rows nparts=4 prefix=3"],
         spared_cases=["sha512_rows nparts=1 prefix=3"],
         edits=[("parts.len.data(), parts.ptr.size(), out64, n)", "parts.len.data(), parts.len[0], out64, n)")]),
    dict(name="sum_rows_terms_and_n_exchanged", wrappers={"sum_rows_ed"}, cases=["sum_rows_ed n=3 t=33", "sum_rows_ed n=3 t=0"], calls_only=True,
         edits=[("p.data(), terms, o.data(), n), \"zc_ed_sum_rows\")", "p.data(), n, o.data(), terms), \"zc_ed_sum_rows\")")]),
    dict(name="generators_move_assign_leaks", wrappers={"Generators"}, cases=["Generators move_assign"], spared_cases=["Generators move"],
         edits=[("            reset();\n            id_ = o.id_;\n            count_ = o.count_;", "            id_ = o.id_;\n            count_ = o.count_;")]),
]
BY_NAME = {m["name"]: m for m in MUTANTS}


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    base = str(tmp_path_factory.mktemp("mirror_calls"))
    assert not base.startswith(ROOT + os.sep)
    lib = os.path.dirname(build_standin(os.path.join(base, "lib")))
    jobs = [(None, (), ())] + [(m["name"], m["edits"], ()) for m in MUTANTS]
    san = sanitizers_link(base)
    if san:
        jobs.append(("sanitized", (), SAN))

    def job(j):
        name, edits, flags = j
        libdir = os.path.dirname(build_standin(os.path.join(base, "lib_san"), SAN)) if flags else lib
        return build_driver(os.path.join(base, name or "unmutated"), libdir, edits, flags)
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        exes = dict(zip([j[0] for j in jobs], pool.map(job, jobs)))
    return dict(base=base, exes=exes, sanitized=san)


@pytest.fixture(scope="module")
def clean_run(built):
    return run_driver(built["exes"][None], built["base"])


def test_shape_table_names_every_pointer_of_every_prototype():
    SI.source(PROTOS, SHAPES)                                  # asserts: every pointer has a shape, every shape a pointer
    assert len(PROTOS) == len(ARGS) >= 92
    with pytest.raises(AssertionError, match="no shape for pointer rows of zc_fe_new"):
        SI.source(all_prototypes("int zc_fe_new(zc_ctx *ctx, const uint64_t *rows, size_t n);"), SHAPES)


def test_every_wrapper_calls_what_the_headers_say(clean_run):
    assert clean_run.returncode == 0, clean_run.stderr
    assert failures(clean_run) == []


def referenced(hpp_text):
    return set(re.findall(r"\b(zc_[a-z0-9_]+)\s*\(", hpp_text))


def coverage_gaps(logged, hpp_text, protos):
    """(symbols the headers declare or the mirror references that no record names, symbols the mirror references that no header declares)"""
    declared = {name for name, _ in protos}
    return sorted((declared | referenced(hpp_text)) - set(logged)), sorted(referenced(hpp_text) - declared)


def test_the_log_covers_every_symbol(clean_run):
    logged = {sym for _, records in clean_run.log for sym, _ in records}
    hpp = open(HPP).read()
    assert coverage_gaps(logged, hpp, PROTOS) == ([], [])
    assert len(logged) == len(ARGS) >= 92
    # a prototype added to a header without a call in the driver, a wrapper over a new symbol without one
    assert coverage_gaps(logged, hpp, all_prototypes("int zc_fe_cube(zc_ctx *ctx, const uint64_t *a, uint64_t *out, size_t n);"))[0] == ["zc_fe_cube"]
    grown = hpp + '\ninline void cube() { Backend::check(zc_fe_cube(Backend::ctx(), nullptr, nullptr, 0), "zc_fe_cube"); }\n'
    assert coverage_gaps(logged, grown, PROTOS) == (["zc_fe_cube"], ["zc_fe_cube"])


def test_every_wrapper_over_vectors_has_a_buffer_check(clean_run):
    """every function of the mirror that takes a std::vector is the wrapper of a segment whose expected record holds input bytes"""
    hpp = open(HPP).read()
    takers = set(re.findall(r"(\w+)\(\s*const std::vector<", hpp))
    assert {"ed_lincomb", "ris_lincomb_sum", "msm", "sum_rows", "MsmBases", "Generators", "mul", "mul_compress", "flat", "fold_ordered"} <= takers
    alias = {"mul_batch_fe": "mul_batch", "sum_rows_ed": "sum_rows", "sum_rows_wire": "sum_rows"}
    checked = set()
    ids = Ids()
    for label, _ in clean_run.log:
        name, p = parse_label(label)
        calls, _ = EXPECT[name](p, ids)
        for sym, want in (calls[1] if isinstance(calls, tuple) else calls):
            if any(isinstance(v, str) and len(v) >= 80 and re.fullmatch(r"[0-9a-f]+", v) for v in want.values()):
                checked.add(alias.get(name, name).split("::")[-1])
                if name in ("MsmBases", "Generators"):      # the members of the handle classes run inside the class's segments
                    checked |= {"zc_msm_fixed": {"msm"}, "zc_ed_mul_gens": {"mul", "flat"}, "zc_ris_mul_gens_compress": {"mul_compress", "flat"}}.get(sym, set())
    assert takers - checked == set()


def test_a_failing_status_throws_and_names_the_symbol(built):
    """Backend::check: std::runtime_error with the symbol and zc_last_error(), for every call whose status the mirror checks"""
    exe = built["exes"][None]
    checked = sorted(set(ARGS) - UNCHECKED)

    def one(sym):
        r = run_driver(exe, built["base"], {"ZC_STANDIN_FAIL": sym})
        want = "! runtime_error %s failed: %s" % (sym, SI.LAST_ERROR)
        for (label, printed), (_, records) in zip(r.out, r.log):
            if any(s == sym for s, _ in records):
                return None if want in printed else "%s: the first call, in %r, printed %r" % (sym, label, printed[:2])
        return "%s: never called" % sym
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        assert [m for m in pool.map(one, checked) if m] == []


def test_catalogue_is_sound():
    text = open(HPP).read()
    assert len(BY_NAME) == len(MUTANTS) >= 8
    for m in MUTANTS:
        for old, new in m["edits"]:
            assert text.count(old) == 1 and old != new, m["name"]


@pytest.mark.parametrize("name", [m["name"] for m in MUTANTS])
def test_planted_defect_is_caught(built, name):
    m = BY_NAME[name]
    calls_only = m.get("calls_only", False)
    run = run_driver(built["exes"][name], built["base"], {"ZC_STANDIN_NOFILL": "1"} if calls_only else None)
    bad = failures(run, returns=not calls_only)
    assert bad != [], "%s survived" % name
    failed = {b.split(": ", 1)[0] for b in bad}                 # (a label holds "::" but never ": ")
    assert {parse_label(label)[0] for label in failed} == m["wrappers"], bad
    for case in m.get("cases", []):
        assert case in failed, (name, case, sorted(failed))
    for case in m.get("spared_cases", []):
        assert case not in failed, (name, case, sorted(failed))


def test_sanitized_build_runs_clean(built):
    """the same program and stand-in under AddressSanitizer and UBSan: the wrappers size their own vectors, and the stand-in reads
    every extent in full"""
    if not built["sanitized"]:
        pytest.skip("gcc's sanitizer runtimes are not installed")
    run = run_driver(built["exes"]["sanitized"], built["base"], {"ASAN_OPTIONS": "detect_leaks=0"})
    assert run.returncode == 0, run.stderr[-2000:]
    assert failures(run) == []


def test_nothing_is_left_in_the_tree(built):
    assert not any(p.startswith(ROOT + os.sep) for p in built["exes"].values())
    assert not os.path.exists(os.path.join(HERE, "cpp", "mirror_calls")) and not os.path.exists(os.path.join(HERE, "cpp", "libzerocaf_hip.so"))
