"""CPU tier: zc_ris_double_and_compress is declared in the second public header (include/zerocaf_hip_ext.h: additive entry
points beyond the 0.6 table), exported by both libraries, bound in Python beside the 0.6 table and not inside it, refuses a
missing pointer by name before the context is touched, and reaches the library from the Engine with the right symbol,
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
NAME = "zc_ris_double_and_compress"
PROTOTYPE = "int zc_ris_double_and_compress(zc_ctx *ctx, const uint64_t *p, uint8_t *out32, size_t n);"
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


def test_the_second_header_declares_it_and_the_first_keeps_its_92_names():
    ext, main = open(EXT_HEADER).read(), open(HEADER).read()
    assert "additive entry points beyond the 0.6 table" in ext and '#include "zerocaf_hip.h"' in ext
    decls = " ".join(re.sub(r"/\*.*?\*/", "", ext, flags=re.S).split())
    assert " ".join(PROTOTYPE.split()) in decls
    assert _names(ext) == {NAME}
    assert len(_names(main)) == 92 and NAME not in main
    for word in ("32 zero bytes", "by value", "null pointer: p", "null pointer: out32", "null context", "ZC_ERR_MIXED_MEM", "8-byte alignment", "must not overlap"):
        assert word.lower() in " ".join(ext.split()).lower(), word


def test_the_second_header_is_plain_c11(tmp_path):
    """Compiled as C11 with warnings as errors, and the prototype is the one a C caller links against."""
    src = tmp_path / "t.c"
    src.write_text('#include "zerocaf_hip_ext.h"\n'
                   "int (*const fp)(zc_ctx *, const uint64_t *, uint8_t *, size_t) = zc_ris_double_and_compress;\n"
                   "int main(void) { return fp(0, 0, 0, 0) == ZC_ERR_BAD_ARG ? 0 : 1; }\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-c", "-o", str(tmp_path / "t.o"), str(src)])


def test_both_libraries_export_it_and_python_binds_it_beside_the_table(lib):
    import dusk_zerocaf_amd as z
    from dusk_zerocaf_amd import _lib
    for path in (z.LIB_PATH, _lib.TEST_LIB_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        assert NAME in set(re.findall(r"\bT (zc_[a-z0-9_]+)", out)), path
    assert list(_lib.EXT_SIGNATURES) == [NAME] and _lib.EXT_SIGNATURES[NAME] == [C.c_void_p, C.c_void_p, C.c_size_t]
    assert NAME not in z.ALL_SYMBOLS and NAME not in _lib.SIGNATURES and NAME not in _lib.SCALAR_EXT_SIGNATURES
    fn = getattr(lib, NAME)
    assert fn.restype is C.c_int and len(fn.argtypes) == 4
    assert lib.zc_version().decode().startswith("zerocaf_hip 0.6 ")                  # additive: the ABI number stays


def test_a_missing_pointer_is_refused_by_name_before_the_context_is_touched(lib):
    """ctx = NULL throughout: with both pointers present the call gets as far as the context ("null context"); with one of
    them NULL it is ZC_ERR_BAD_ARG with the message that names it, for n = 0 too."""
    p, out = np.zeros(40, dtype=np.uint64), np.zeros(64, dtype=np.uint8)
    full = [C.c_void_p(p.ctypes.data), C.c_void_p(out.ctypes.data)]
    fn = getattr(lib, NAME)
    for n in (1, 0):
        assert fn(None, *full, n) == ZC_ERR_BAD_ARG and lib.zc_last_error() == b"null context"
        for i, pname in enumerate(("p", "out32")):
            args = list(full)
            args[i] = None
            assert fn(None, *args, n) == ZC_ERR_BAD_ARG
            assert lib.zc_last_error().decode() == "null pointer: %s" % pname
    assert not p.any() and not out.any()


@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_the_engine_method_calls_the_library_as_the_header_says(kind):
    """One call: the symbol, then ctx, p, out32, n; the output is of the input's kind, (n, 32) uint8."""
    from dusk_zerocaf_amd import engine
    n = 3
    e, rec = _gen().new_engine(engine)
    try:
        p = np.arange(n * 20, dtype=np.uint64).reshape(n, 20)
        if kind == "torch":
            import torch
            p = torch.from_numpy(p.view(np.int64))
        got = e.ris_double_and_compress(p)
        ptr = lambda x: x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()
        assert len(rec.calls) == 1 and rec.calls[0][0] == NAME
        args = rec.calls[0][1]
        assert args[0] is e.ctx and list(args[1:]) == [ptr(p), ptr(got), n]
        assert tuple(got.shape) == (n, 32) and "uint8" in str(got.dtype) and isinstance(got, np.ndarray) == (kind == "numpy")
        with pytest.raises(AssertionError):
            e.ris_double_and_compress(np.zeros((n, 10), dtype=np.uint64))          # not a point record
        assert len(rec.calls) == 1
    finally:
        e.ctx = None


def test_the_method_lives_on_a_base_class_of_engine():
    """The recorded method table of tests/test_engine_calls.py lists what `class Engine` itself defines."""
    from dusk_zerocaf_amd import engine, ristretto_batch
    assert issubclass(engine.Engine, ristretto_batch.RistrettoBatchMixin)
    assert "ris_double_and_compress" not in vars(engine.Engine) and callable(engine.Engine.ris_double_and_compress)


def test_cpp_and_rust_mirrors_and_documents():
    rd = lambda *parts: open(os.path.join(ROOT, *parts)).read()
    hpp = rd("dusk_zerocaf_amd", "include", "zerocaf.hpp")
    rust = os.path.join("integration", "rust", "zerocaf-hip", "src")
    ext_rs, lib_rs, ffi = rd(rust, "ext.rs"), rd(rust, "lib.rs"), rd(rust, "ffi.rs")
    readme, integ, design = rd("README.md"), rd("INTEGRATION.md"), rd("DESIGN.md")
    assert "zerocaf_hip_ext.h" in hpp and NAME + "(" in hpp
    assert 'extern "C"' in ext_rs and "pub fn " + NAME + "(" in ext_rs and "pub fn ris_double_and_compress(" in ext_rs
    assert re.search(r"^pub mod ext;$", lib_rs, flags=re.M) and NAME not in lib_rs and NAME not in ffi
    for doc in (readme, integ, design):
        assert NAME in doc and "zerocaf_hip_ext.h" in doc
    assert "92 entry points" in readme and "**all 92** entry points" in integ and "\n92 entry points (" in integ
    assert "zc_sc_muladd" in integ[integ.index(NAME):] and "order L" in integ                 # the k/2 mod L recipe
    assert "k_ris_double_compress_chunked" in design and "zc_ris_batch.hip.h" in design and "VGPR" in design
    assert "zc_ris_batch.hip.h" in rd("dusk_zerocaf_amd", "build.py")
