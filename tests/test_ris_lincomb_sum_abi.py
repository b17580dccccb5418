"""CPU tier: zc_ris_lincomb_sum is declared with its contract in include/zerocaf_hip_ext_sum.h, the part of the second public
header (include/zerocaf_hip_ext.h, which includes it) for calls that reduce a batch to one result,
exported by both libraries, bound in Python beside the 0.6 table and not inside it, refuses its arguments -- a missing
pointer by name, terms == 0, a batch beyond the MSM's index limits -- before the context is touched, and reaches the library
from the Engine with the right symbol, argument order, shapes and dtypes.  (No GPU: the library calls fail on their arguments,
the Engine calls go to a recording stand-in, as in tests/test_engine_calls.py.)"""
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
SUM_HEADER = os.path.join(ROOT, "include", "zerocaf_hip_ext_sum.h")
NAME = "zc_ris_lincomb_sum"
PROTOTYPE = ("int zc_ris_lincomb_sum(zc_ctx *ctx, const uint8_t *in32, const uint64_t *scalars, size_t terms, const uint64_t *base_scalars, "
             "const uint64_t *weights, uint8_t *out32, uint8_t *ok, size_t n);")
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


def test_the_second_header_declares_it_with_its_contract_and_the_first_keeps_its_92_names():
    ext, main = open(SUM_HEADER).read(), open(HEADER).read()
    outer = re.sub(r"/\*.*?\*/", "", open(EXT_HEADER).read(), flags=re.S)
    assert re.search(r'^#include "zerocaf_hip_ext_sum.h"$', outer, flags=re.M) and '#include "zerocaf_hip.h"' in ext     # one include reaches it
    decls = " ".join(re.sub(r"/\*.*?\*/", "", ext, flags=re.S).split())
    assert " ".join(PROTOTYPE.split()) in decls
    assert _names(ext) == {NAME} and len(_names(main)) == 92 and NAME not in main
    flat = " ".join(ext.split()).lower()
    for word in ("by value", "32 zero bytes", "n == 0", "null pointer: in32", "null context", "terms == 0", "2^31", "ZC_ERR_MIXED_MEM", "8-byte alignment",
                 "host memory", "synchronous", "left out completely", "no byte of any input", "L - c", "128 random bits", "src/ristretto.rs:96-154"):
        assert word.lower() in flat, word


@pytest.mark.parametrize("header", ["zerocaf_hip_ext.h", "zerocaf_hip_ext_sum.h"])
def test_the_headers_are_plain_c11(tmp_path, header):
    """Compiled as C11 with warnings as errors through the second header and on its own; the prototype is the one a C caller
    links against."""
    src = tmp_path / "t.c"
    src.write_text('#include "%s"\n' % header +
                   "int (*const fp)(zc_ctx *, const uint8_t *, const uint64_t *, size_t, const uint64_t *, const uint64_t *, uint8_t *, uint8_t *, size_t) = zc_ris_lincomb_sum;\n"
                   "int main(void) { return fp(0, 0, 0, 1, 0, 0, 0, 0, 0) == ZC_ERR_BAD_ARG ? 0 : 1; }\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-c", "-o", str(tmp_path / "t.o"), str(src)])


def test_both_libraries_export_it_and_python_binds_it_beside_the_table(lib):
    import dusk_zerocaf_amd as z
    from dusk_zerocaf_amd import _lib
    for path in (z.LIB_PATH, _lib.TEST_LIB_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        assert NAME in set(re.findall(r"\bT (zc_[a-z0-9_]+)", out)), path
    vp = C.c_void_p
    assert list(_lib.EXT_SUM_SIGNATURES) == [NAME] and _lib.EXT_SUM_SIGNATURES[NAME] == [vp, vp, C.c_size_t, vp, vp, vp, vp, C.c_size_t]
    assert NAME not in z.ALL_SYMBOLS and NAME not in _lib.SIGNATURES and NAME not in _lib.SCALAR_EXT_SIGNATURES and NAME not in _lib.EXT_SIGNATURES
    fn = getattr(lib, NAME)
    assert fn.restype is C.c_int and len(fn.argtypes) == 9
    assert lib.zc_version().decode().startswith("zerocaf_hip 0.6 ")                  # additive: the ABI number stays


def test_arguments_are_refused_before_the_context_is_touched(lib):
    """ctx = NULL throughout: with good arguments the call gets as far as the context ("null context"), for n = 0 too; a missing
    in32, scalars or out32 is named; terms == 0 and a batch of n terms + 1 >= 2^31 pairs are refused; the optional arrays may
    be missing.  Nothing is written."""
    e, k, s = np.zeros(64, dtype=np.uint8), np.zeros(10, dtype=np.uint64), np.zeros(5, dtype=np.uint64)
    out, ok = np.full(32, 0xA5, dtype=np.uint8), np.full(1, 0xA5, dtype=np.uint8)
    P = lambda a: C.c_void_p(a.ctypes.data)
    fn = getattr(lib, NAME)
    err = lambda: lib.zc_last_error().decode()
    for n in (1, 0):
        for kb, z, m in ((P(s), P(s), P(ok)), (None, None, None)):
            assert fn(None, P(e), P(k), 2, kb, z, P(out), m, n) == ZC_ERR_BAD_ARG and err() == "null context"
            for i, pname in ((0, "in32"), (1, "scalars"), (5, "out32")):
                args = [P(e), P(k), 2, kb, z, P(out), m, n]
                args[i] = None
                assert fn(None, *args) == ZC_ERR_BAD_ARG and err() == "null pointer: %s" % pname
            assert fn(None, P(e), P(k), 0, kb, z, P(out), m, n) == ZC_ERR_BAD_ARG and "terms must be at least 1" in err()
    # the limit: n * terms + 1 pairs must stay below 2^31
    full = (P(e), P(k))
    for terms, n, refused in ((1, (1 << 31) - 1, True), (1, (1 << 31) - 2, False), (2, 1 << 30, True), (2, (1 << 30) - 1, False), (7, (1 << 31) // 7 + 1, True),
                              (3, 1 << 62, True), (1 << 40, 1 << 40, True), ((1 << 64) - 1, 2, True), ((1 << 31) - 2, 1, False), ((1 << 31) - 1, 1, True)):
        assert fn(None, *full, terms, P(s), P(s), P(out), P(ok), n) == ZC_ERR_BAD_ARG
        assert ("below 2^31" in err()) == refused and (refused or err() == "null context"), (terms, n, err())
    assert not e.any() and not k.any() and not s.any() and (out == 0xA5).all() and (ok == 0xA5).all()


@pytest.mark.parametrize("kind", ["numpy", "torch"])
@pytest.mark.parametrize("base,weights", [(False, False), (True, False), (False, True), (True, True)])
def test_the_engine_method_calls_the_library_as_the_header_says(kind, base, weights):
    """One call: the symbol, then ctx, in32, scalars, terms, base_scalars, weights, out32 (host memory), ok, n; the bytes come
    back as `bytes`, the mask as an array of the inputs' kind."""
    from dusk_zerocaf_amd import engine
    n, t = 3, 2
    e, rec = _gen().new_engine(engine)
    try:
        conv = lambda a: a
        if kind == "torch":
            import torch
            conv = lambda a: torch.from_numpy(a if a.dtype == np.uint8 else a.view(np.int64))
        E = conv(np.arange(n * t * 32, dtype=np.uint8).reshape(n, t, 32))
        K = conv(np.arange(n * t * 5, dtype=np.uint64).reshape(n, t, 5))
        KB = conv(np.arange(n * 5, dtype=np.uint64).reshape(n, 5)) if base else None
        Z = conv(np.arange(n * 5, dtype=np.uint64).reshape(n, 5)) if weights else None
        got, ok = e.ris_lincomb_sum(E, K, KB, Z)
        ptr = lambda x: None if x is None else x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()
        assert len(rec.calls) == 1 and rec.calls[0][0] == NAME
        args = rec.calls[0][1]
        assert args[0] is e.ctx and list(args[1:6]) == [ptr(E), ptr(K), t, ptr(KB), ptr(Z)] and list(args[7:]) == [ptr(ok), n]
        assert isinstance(args[6], int) and args[6] not in (0, ptr(ok))                  # a host buffer of the call's own
        assert isinstance(got, bytes) and len(got) == 32
        assert tuple(ok.shape) == (n,) and "uint8" in str(ok.dtype) and isinstance(ok, np.ndarray) == (kind == "numpy")
        with pytest.raises(AssertionError):
            e.ris_lincomb_sum(E, K[:, :1])                                                # term counts differ
        if base:
            with pytest.raises(AssertionError):
                e.ris_lincomb_sum(E, K, KB[:2], Z)                                        # row counts differ
        if kind == "torch":
            with pytest.raises(AssertionError):
                e.ris_lincomb_sum(E, K, np.zeros((n, 5), dtype=np.uint64))                # numpy beside tensors
        assert len(rec.calls) == 1
    finally:
        e.ctx = None


def test_the_method_lives_on_a_base_class_of_engine():
    """The recorded method table of tests/test_engine_calls.py lists what `class Engine` itself defines."""
    from dusk_zerocaf_amd import engine, ristretto_batch
    assert issubclass(engine.Engine, ristretto_batch.RistrettoBatchMixin)
    assert "ris_lincomb_sum" not in vars(engine.Engine) and callable(engine.Engine.ris_lincomb_sum)


def _rust_decl(text, name):
    m = re.search(r"pub fn %s\((.*?)\)\s*->\s*c_int;" % name, text, flags=re.S)
    assert m, name
    return [tuple(x.strip() for x in p.split(":")) for p in m.group(1).split(",")]


def test_the_rust_declaration_matches_the_header():
    """Parameter for parameter: names, constness, pointee width."""
    rd = lambda *parts: open(os.path.join(ROOT, *parts)).read()
    rust = os.path.join("integration", "rust", "zerocaf-hip", "src")
    ext_rs, lib_rs, ffi = rd(rust, "ext.rs"), rd(rust, "lib.rs"), rd(rust, "ffi.rs")
    params = re.search(r"%s\((.*?)\);" % NAME, " ".join(PROTOTYPE.split())).group(1).split(",")
    ctypes_to_rust = {"zc_ctx *": "*mut ZcCtx", "const uint8_t *": "*const u8", "const uint64_t *": "*const u64", "uint8_t *": "*mut u8", "size_t ": "usize"}
    want = []
    for p in params:
        p = p.strip()
        nm = re.search(r"([a-z0-9_]+)$", p).group(1)
        want.append((nm, ctypes_to_rust[p[:len(p) - len(nm)]]))
    assert _rust_decl(ext_rs, NAME) == want
    assert "pub fn ris_lincomb_sum(" in ext_rs and re.search(r"^pub mod ext;$", lib_rs, flags=re.M) and NAME not in lib_rs and NAME not in ffi


def test_cpp_mirror_and_documents():
    rd = lambda *parts: open(os.path.join(ROOT, *parts)).read()
    hpp = rd("dusk_zerocaf_amd", "include", "zerocaf.hpp")
    readme, integ, design = rd("README.md"), rd("INTEGRATION.md"), rd("DESIGN.md")
    assert "zerocaf_hip_ext.h" in hpp and NAME + "(" in hpp and "zerocaf_hip_ext_sum.h" in rd("dusk_zerocaf_amd", "build.py") and "ris_lincomb_sum(" in hpp
    for doc in (readme, integ, design):
        assert NAME in doc and "zerocaf_hip_ext_sum.h" in doc
    assert "92 entry points" in readme and "tools/bench_ris_lincomb_sum.py" in readme and "profiles/r14_ris_lincomb_sum.json" in readme
    recipe = integ[integ.index(NAME):]
    assert "L - c" in recipe and "128" in recipe and re.search(r"every\s+`?ok`?\s+is\s+1", recipe)
    for word in ("k_ris_sum_prepare", "k_ris_sum_rows", "k_sc_sum", "msm_on_device", "zc_ris_batch.hip.h"):
        assert word in design, word
    src = rd("dusk_zerocaf_amd", "csrc", "zerocaf_hip.hip")
    body = src[src.index("int zc_ris_lincomb_sum("):]
    body = body[:body.index("\n}\n")]
    for kernel in ("k_ris_sum_prepare", "k_ris_sum_rows", "k_sc_sum", "k_ris_compress"):          # every new __global__ has its launch site here
        assert "hipLaunchKernelGGL(zc::%s," % kernel in body, kernel
    assert "msm_on_device(D, wP, wK, count, &res)" in body
