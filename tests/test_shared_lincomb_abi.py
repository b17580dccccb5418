"""CPU tier: zc_ed_lincomb_shared and zc_ris_lincomb_shared are declared with their contract in
include/zerocaf_hip_ext_shared_lincomb.h, which include/zerocaf_hip_ext.h includes on the line after zerocaf_hip_ext_shared.h;
exported by both libraries; bound in Python beside the 0.6 table and not inside it; refuse a missing pointer by name, a term
count outside 1..8 and n * terms >= 2^31 before the context is touched; reach the library from the Engine with the right symbol,
argument order, shapes and dtypes.  (No GPU: the library calls fail on their arguments, the Engine calls go to a recording
stand-in, as in tests/test_engine_calls.py.)"""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zerocaf_hip.h")
EXT_HEADER = os.path.join(ROOT, "include", "zerocaf_hip_ext.h")
SHARED_HEADER = os.path.join(ROOT, "include", "zerocaf_hip_ext_shared.h")
LINCOMB_HEADER = os.path.join(ROOT, "include", "zerocaf_hip_ext_shared_lincomb.h")
ED, RIS = "zc_ed_lincomb_shared", "zc_ris_lincomb_shared"
PROTOTYPES = ["int zc_ed_lincomb_shared(zc_ctx *ctx, const uint64_t *points, const uint64_t *k, size_t terms, uint64_t *out, size_t n);",
              "int zc_ris_lincomb_shared(zc_ctx *ctx, const uint8_t *in32, const uint64_t *k, size_t terms, uint8_t *out32, uint8_t *ok, size_t n);"]
ZC_ERR_BAD_ARG = -1


@pytest.fixture(scope="module")
def lib():
    import dusk_zerocaf_amd as z
    if not os.path.exists(z.LIB_PATH):
        from dusk_zerocaf_amd import build
        build.build(test_hooks=True)
    return z.load()


def _gen():
    spec = importlib.util.spec_from_file_location("gen_engine_calls", os.path.join(ROOT, "tests", "golden", "gen_engine_calls.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def _names(text):
    return set(re.findall(r"\b(zc_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


def test_the_header_declares_exactly_the_two_prototypes_and_comes_in_after_the_shared_one():
    lh, sh, ext, main = open(LINCOMB_HEADER).read(), open(SHARED_HEADER).read(), open(EXT_HEADER).read(), open(HEADER).read()
    decls = " ".join(re.sub(r"/\*.*?\*/", "", lh, flags=re.S).split())
    for proto in PROTOTYPES:
        assert " ".join(proto.split()) in decls
    assert _names(lh) == {ED, RIS} and '#include "zerocaf_hip.h"' in lh
    outer = re.sub(r"/\*.*?\*/", "", ext, flags=re.S)
    assert re.search(r'^#include "zerocaf_hip_ext_shared.h"\n#include "zerocaf_hip_ext_shared_lincomb.h"\n', outer, flags=re.M)
    assert len(_names(ext)) == 1 and len(_names(main)) == 92 and len(_names(sh)) == 2
    for other in (main, ext, sh):
        assert ED not in other and RIS not in other
    flat = " ".join(lh.replace("\n *", "\n").split()).lower()                     # the comment's text without its line prefixes
    for word in ("one scalar vector", "host memory", "k must be host memory", "may overwrite k", "early-stop", "depends on k", "zc_scalar_mul_fast",
                 "not by k_j mod l", "no second strict pass", "out must not overlap points unless terms == 1", "zc_ed_scalar_mul_shared", "zc_ris_mul_shared",
                 "base_scalars = null", "ok may be null", "zc_ristretto_strict", "32 zero bytes", "no basepoint term", "encoding of b as a term",
                 "null pointer: points", "null pointer: k", "null pointer: out", "null pointer: in32", "null pointer: out32", "null context",
                 "zc_lincomb_max_terms", "2^31", "zc_err_mixed_mem", "keeps no copy", "rows 0 .. n-1", "no environment knob", "row-major like zc_ed_lincomb",
                 "row-major like zc_ris_lincomb"):
        assert word in flat, word


@pytest.mark.parametrize("header", ["zerocaf_hip_ext.h", "zerocaf_hip_ext_shared_lincomb.h"])
def test_the_header_is_plain_c11(tmp_path, header):
    """Compiled as C11 with warnings as errors, alone and through the outer header; the prototypes are the ones a C caller links against."""
    src = tmp_path / "t.c"
    src.write_text('#include "%s"\n' % header +
                   "int (*const fe)(zc_ctx *, const uint64_t *, const uint64_t *, size_t, uint64_t *, size_t) = zc_ed_lincomb_shared;\n"
                   "int (*const fr)(zc_ctx *, const uint8_t *, const uint64_t *, size_t, uint8_t *, uint8_t *, size_t) = zc_ris_lincomb_shared;\n"
                   "int main(void) { return fe(0, 0, 0, ZC_LINCOMB_MAX_TERMS, 0, 0) == ZC_ERR_BAD_ARG && fr(0, 0, 0, 1, 0, 0, 0) == ZC_ERR_BAD_ARG ? 0 : 1; }\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-c", "-o", str(tmp_path / "t.o"), str(src)])


def test_both_libraries_export_them_and_python_binds_them_beside_the_table(lib):
    import dusk_zerocaf_amd as z
    from dusk_zerocaf_amd import _lib
    for path in (z.LIB_PATH, _lib.TEST_LIB_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        assert {ED, RIS} <= set(re.findall(r"\bT (zc_[a-z0-9_]+)", out)), path
        assert not [s for s in re.findall(r"\bT (zc_test_[a-z0-9_]+)", out) if "lincomb_shared" in s or "shared_lincomb" in s]
    v, n = C.c_void_p, C.c_size_t
    assert list(_lib.EXT_SHARED_LINCOMB_SIGNATURES) == [ED, RIS]
    assert _lib.EXT_SHARED_LINCOMB_SIGNATURES[ED] == [v, v, n, v, n] and _lib.EXT_SHARED_LINCOMB_SIGNATURES[RIS] == [v, v, n, v, v, n]
    assert list(_lib.EXT_SHARED_SIGNATURES) == ["zc_ed_scalar_mul_shared", "zc_ris_mul_shared"]
    for name in (ED, RIS):
        assert name not in z.ALL_SYMBOLS
        for table in (_lib.SIGNATURES, _lib.SCALAR_EXT_SIGNATURES, _lib.EXT_SIGNATURES, _lib.EXT_SUM_SIGNATURES, _lib.EXT_HASH_SIGNATURES, _lib.EXT_SHARED_SIGNATURES):
            assert name not in table
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(_lib.EXT_SHARED_LINCOMB_SIGNATURES[name]) + 1
    assert lib.zc_version().decode().startswith("zerocaf_hip 0.6 ")                  # additive: the ABI number stays


def test_refusals_come_by_name_and_in_order_before_the_context_is_touched(lib):
    """ctx = NULL throughout: with every argument in order the call gets as far as the context ("null context"), for n = 0 too;
    a NULL pointer is named, the first in the header's order when several are missing; then the term count, then n * terms."""
    p, k, out = np.zeros(160, dtype=np.uint64), np.zeros(40, dtype=np.uint64), np.zeros(40, dtype=np.uint64)
    e, o32, ok = np.zeros(256, dtype=np.uint8), np.zeros(64, dtype=np.uint8), np.zeros(2, dtype=np.uint8)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    err = lambda: lib.zc_last_error().decode()
    for name, ins, outs, pnames in ((ED, [ptr(p), ptr(k)], [ptr(out)], ("points", "k", "out")), (RIS, [ptr(e), ptr(k)], [ptr(o32), ptr(ok)], ("in32", "k", "out32"))):
        fn = getattr(lib, name)
        call = lambda args, terms, n: fn(None, args[0], args[1], terms, *args[2:], n)
        full = ins + outs
        for n in (1, 0):
            assert call(full, 2, n) == ZC_ERR_BAD_ARG and err() == "null context"
            for i, pname in enumerate(pnames):
                args = list(full)
                args[i] = None
                for terms in (2, 0, 9):                                               # the pointer is named before the term count is looked at
                    assert call(args, terms, n) == ZC_ERR_BAD_ARG and err() == "null pointer: %s" % pname
            assert call([None] * len(full), 2, n) == ZC_ERR_BAD_ARG and err() == "null pointer: %s" % pnames[0]
            for terms in (0, 9, 1 << 40):
                assert call(full, terms, n) == ZC_ERR_BAD_ARG and err() == "%s: terms must be 1..ZC_LINCOMB_MAX_TERMS" % name
        for terms in range(1, 9):
            assert call(full, terms, 8) == ZC_ERR_BAD_ARG and err() == "null context"
            edge = -(-(1 << 31) // terms)                                              # the first n with n * terms >= 2^31
            assert call(full, terms, edge) == ZC_ERR_BAD_ARG and err() == "%s: n * terms must stay below 2^31" % name
            assert call(full, terms, edge - 1) == ZC_ERR_BAD_ARG and err() == "null context"
        assert call(full, 1, 1 << 31) == ZC_ERR_BAD_ARG and "2^31" in err() and call(full, 8, 1 << 28) == ZC_ERR_BAD_ARG and "2^31" in err()
    assert lib.zc_ris_lincomb_shared(None, ptr(e), ptr(k), 2, ptr(o32), None, 1) == ZC_ERR_BAD_ARG and err() == "null context"      # ok may be NULL
    assert not p.any() and not out.any() and not o32.any() and not ok.any()


@pytest.mark.parametrize("kind", ["numpy", "torch"])
@pytest.mark.parametrize("scalar", ["words", "ints"])
def test_the_engine_methods_call_the_library_as_the_header_says(kind, scalar):
    """One call each: the symbol, then ctx, the rows, k (terms * 5 host words), terms, the outputs, n; outputs of the input's kind."""
    from dusk_zerocaf_amd import engine
    n, t = 3, 2
    e, rec = _gen().new_engine(engine)
    try:
        p = np.arange(n * t * 20, dtype=np.uint64).reshape(n, t, 20)
        enc = np.arange(n * t * 32, dtype=np.uint8).reshape(n, t, 32)
        kvs = [0x123456789ABCDEF0123456789ABCDEF0123456789, 7]
        words = [[(kv >> (52 * i)) & ((1 << 52) - 1) for i in range(5)] for kv in kvs]
        k = np.array(words, dtype=np.uint64) if scalar == "words" else kvs
        if kind == "torch":
            import torch
            p, enc = torch.from_numpy(p.view(np.int64)), torch.from_numpy(enc)
        ptr = lambda x: x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()
        read_k = lambda a: list((C.c_uint64 * (5 * t)).from_address(a.value))

        seen = []
        real = rec.__getattr__

        class Peek:
            """The scalars' words as they are when the library is called (the mixin owns the array only for the call)."""
            def __getattr__(self, name):
                fn = real(name)

                def wrapped(*args):
                    seen.append(read_k(args[2]))
                    return fn(*args)
                return wrapped
        e.lib = Peek()
        got = e.ed_lincomb_shared(p, k)
        out32, ok = e.ris_lincomb_shared(enc, k)
        assert [c[0] for c in rec.calls] == [ED, RIS] and seen == [words[0] + words[1]] * 2
        a = rec.calls[0][1]
        assert a[0] is e.ctx and [a[1], a[3], a[4], a[5]] == [ptr(p), t, ptr(got), n] and isinstance(a[2], C.c_void_p)
        b = rec.calls[1][1]
        assert b[0] is e.ctx and [b[1], b[3], b[4], b[5], b[6]] == [ptr(enc), t, ptr(out32), ptr(ok), n] and isinstance(b[2], C.c_void_p)
        assert tuple(got.shape) == (n, 20) and tuple(out32.shape) == (n, 32) and tuple(ok.shape) == (n,)
        assert "uint8" in str(out32.dtype) and "uint8" in str(ok.dtype) and "int64" in str(got.dtype)
        for x in (got, out32, ok):
            assert isinstance(x, np.ndarray) == (kind == "numpy")
        with pytest.raises(AssertionError):
            e.ed_lincomb_shared(np.zeros((n, 20), dtype=np.uint64), k)                # rows without a term dimension
        with pytest.raises(AssertionError):
            e.ris_lincomb_shared(enc, np.zeros((3, 5), dtype=np.uint64))              # three scalars for two terms
        with pytest.raises(AssertionError):
            e.ris_lincomb_shared(enc, [1, 1 << 260])
        assert len(rec.calls) == 2
    finally:
        e.ctx = None


def test_the_methods_live_on_a_base_class_of_engine():
    """The recorded method table of tests/test_engine_calls.py lists what `class Engine` itself defines."""
    from dusk_zerocaf_amd import engine, shared_scalar
    assert issubclass(engine.Engine, shared_scalar.SharedScalarMixin)
    for m in ("ed_lincomb_shared", "ris_lincomb_shared"):
        assert m not in vars(engine.Engine) and m in vars(shared_scalar.SharedScalarMixin) and callable(getattr(engine.Engine, m))


def test_cpp_and_rust_mirrors_and_documents():
    rd = lambda *parts: open(os.path.join(ROOT, *parts)).read()
    hpp = rd("dusk_zerocaf_amd", "include", "zerocaf.hpp")
    rust = os.path.join("integration", "rust", "zerocaf-hip", "src")
    ext_rs, lib_rs, ffi = rd(rust, "ext.rs"), rd(rust, "lib.rs"), rd(rust, "ffi.rs")
    readme, integ, design = rd("README.md"), rd("INTEGRATION.md"), rd("DESIGN.md")
    for name in (ED, RIS):
        assert name + "(" in hpp and "pub fn " + name + "(" in ext_rs and "pub fn " + name[3:] + "(" in ext_rs
        assert name not in lib_rs and name not in ffi
        for doc in (readme, integ, design):
            assert name in doc
    for doc in (readme, integ, design):
        assert "zerocaf_hip_ext_shared_lincomb.h" in doc
    assert "92 entry points" in readme and "**all 92** entry points" in integ and "\n92 entry points (" in integ
    assert "### 4j" in integ
    worked = integ[integ.index("### 4j"):]
    for word in ("ElGamal", "zc_sc_neg", "(1, -x mod L)", "threshold", "Lagrange", ED, RIS):
        assert word in worked, word
    assert "### 4.9" in design
    sec = design[design.index("### 4.9"):]
    for word in ("zc_shared.hip.h", "zc_shared_scalar.h", "shared_lincomb_schedule", "k_ed_lincomb_shared", "k_ris_lincomb_shared", "VGPR", "kernel_resources.py",
                 "r19_shared_lincomb.json", "queue"):
        assert word in sec, word
    assert "r19_shared_lincomb.json" in readme and os.path.exists(os.path.join(ROOT, "profiles", "r19_shared_lincomb.json"))
    from dusk_zerocaf_amd import build
    assert any(d.endswith("zerocaf_hip_ext_shared_lincomb.h") for d in build.DEPS)                          # the embedded source hash covers it


def test_no_new_knob_in_the_product(lib):
    """`strings` of the product: the ZC_* knobs are the ten of tests/test_abi.py, none for these calls."""
    import dusk_zerocaf_amd as z
    found = set(re.findall(rb"\x00(ZC_[A-Z][A-Z_0-9]+)(?=\x00)", open(z.LIB_PATH, "rb").read()))
    knobs = sorted(x.decode() for x in found if not x.startswith((b"ZC_ERR", b"ZC_OK")))
    assert knobs == ["ZC_HOST_CHUNKS", "ZC_INV_CHUNK", "ZC_JACOBI_ROUNDS", "ZC_MSM_AFFINE", "ZC_MSM_GROUPS", "ZC_MSM_WINDOW", "ZC_RCCL_PATH",
                     "ZC_RING_SLOTS", "ZC_RISTRETTO_STRICT", "ZC_SCHED"], knobs
