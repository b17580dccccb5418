"""CPU tier: zc_sc_from_bytes_wide, zc_sc_from_bytes_mod_order, zc_sc_muladd and zc_sc_invert are declared, exported by both
libraries, bound in Python, refuse a missing pointer by name before the context is touched, and reach the library from the
Engine with the right symbol, argument order, shapes and dtypes.  (No GPU: the library calls fail on their arguments, the Engine
calls go to a recording stand-in, as in tests/test_engine_calls.py.)"""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zerocaf_hip.h")

SIGNATURES = {
    "zc_sc_from_bytes_wide": "int zc_sc_from_bytes_wide(zc_ctx *ctx, const uint8_t *in64, uint64_t *out, size_t n);",
    "zc_sc_from_bytes_mod_order": "int zc_sc_from_bytes_mod_order(zc_ctx *ctx, const uint8_t *in32, uint64_t *out, size_t n);",
    "zc_sc_muladd": "int zc_sc_muladd(zc_ctx *ctx, const uint64_t *a, const uint64_t *b, const uint64_t *c, uint64_t *out, size_t n);",
    "zc_sc_invert": "int zc_sc_invert(zc_ctx *ctx, const uint64_t *a, uint64_t *out, uint8_t *ok, size_t n);",
}
# pointer parameters in order, None = optional
POINTERS = {
    "zc_sc_from_bytes_wide": ["in64", "out"],
    "zc_sc_from_bytes_mod_order": ["in32", "out"],
    "zc_sc_muladd": ["a", "b", "c", "out"],
    "zc_sc_invert": ["a", "out", None],
}
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


def test_header_declares_the_four_entry_points():
    text = open(HEADER).read()
    assert re.search(r"^\s*ZC_ERR_BAD_ARG\s*=\s*-1\b", text, flags=re.M)
    decls = " ".join(re.sub(r"/\*.*?\*/", "", text, flags=re.S).split())
    for sig in SIGNATURES.values():
        assert " ".join(sig.split()) in decls, sig
    assert len(set(re.findall(r"\b(zc_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))) == 92


def test_both_libraries_export_them_and_python_binds_them(lib):
    import dusk_zerocaf_amd as z
    from dusk_zerocaf_amd import _lib
    for path in (z.LIB_PATH, _lib.TEST_LIB_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        assert set(SIGNATURES) <= set(re.findall(r"\bT (zc_[a-z0-9_]+)", out)), path
    assert set(SIGNATURES) <= set(z.ALL_SYMBOLS) and not set(SIGNATURES) & set(_lib.SIGNATURES)
    assert sorted(_lib.SCALAR_EXT_SIGNATURES) == sorted(SIGNATURES)
    for name in SIGNATURES:
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == 1 + len(_lib.SCALAR_EXT_SIGNATURES[name])
    assert lib.zc_version().decode().startswith("zerocaf_hip 0.6 ")                  # additive: the ABI number stays


@pytest.mark.parametrize("name", sorted(POINTERS))
def test_a_missing_pointer_is_refused_by_name_before_the_context_is_touched(lib, name):
    """ctx = NULL throughout: with every required pointer present the call gets as far as the context ("null context"); with
    one of them NULL it is ZC_ERR_BAD_ARG with the message that names it.  ok = NULL is not refused."""
    ptrs = POINTERS[name]
    bufs = [np.zeros(64, dtype=np.uint64) for _ in ptrs]
    full = [C.c_void_p(b.ctypes.data) for b in bufs]
    fn = getattr(lib, name)
    for n in (1, 0):                                                                  # the pointers are checked before n == 0 returns
        assert fn(None, *full, n) == ZC_ERR_BAD_ARG and lib.zc_last_error() == b"null context"
        for i, pname in enumerate(ptrs):
            args = list(full)
            args[i] = None
            rc = fn(None, *args, n)
            assert rc == ZC_ERR_BAD_ARG
            assert lib.zc_last_error().decode() == ("null pointer: %s" % pname if pname else "null context"), (name, i)
    assert not any(b.any() for b in bufs)


CASES = [("sc_from_bytes_wide", "zc_sc_from_bytes_wide", [(64, np.uint8)], [((5,), "64")]),
         ("sc_from_bytes_mod_order", "zc_sc_from_bytes_mod_order", [(32, np.uint8)], [((5,), "64")]),
         ("sc_muladd", "zc_sc_muladd", [(5, np.uint64)] * 3, [((5,), "64")]),
         ("sc_invert", "zc_sc_invert", [(5, np.uint64)], [((5,), "64"), ((), "uint8")])]


def _arrays(specs, n, kind):
    out = []
    for j, (w, dt) in enumerate(specs):
        a = (np.arange(n * w, dtype=np.uint64) + 100 * j).astype(dt).reshape(n, w)
        if kind == "torch":
            import torch
            a = torch.from_numpy(a if dt == np.uint8 else a.view(np.int64))
        out.append(a)
    return out


def _ptr(x):
    return x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()


@pytest.mark.parametrize("kind", ["numpy", "torch"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_engine_methods_call_the_library_as_the_header_says(case, kind):
    """One call: the symbol, then ctx, the inputs in order, the outputs in order, n; outputs of the inputs' kind with the
    shapes and dtypes of the header's arrays."""
    from dusk_zerocaf_amd import engine
    method, symbol, specs, outs = case
    n = 3
    e, rec = _gen().new_engine(engine)
    try:
        ins = _arrays(specs, n, kind)
        got = getattr(e, method)(*ins)
        got = list(got) if isinstance(got, tuple) else [got]
        assert len(rec.calls) == 1 and rec.calls[0][0] == symbol
        args = rec.calls[0][1]
        assert args[0] is e.ctx
        assert list(args[1:]) == [_ptr(x) for x in ins] + [_ptr(x) for x in got] + [n]          # which array is which
        assert len(got) == len(outs)
        for x, (tail, dt) in zip(got, outs):
            assert tuple(x.shape) == (n,) + tail and dt in str(x.dtype), (x.shape, x.dtype)
            assert isinstance(x, np.ndarray) == (kind == "numpy")
        if method == "sc_muladd":                                                                # the caller's own output, any input
            for which in range(3):
                del rec.calls[:]
                res = e.sc_muladd(*ins, out=ins[which])
                assert res is ins[which] and list(rec.calls[0][1][1:]) == [_ptr(x) for x in ins] + [_ptr(ins[which]), n]
    finally:
        e.ctx = None


def test_engine_refuses_unequal_row_counts_before_any_call():
    from dusk_zerocaf_amd import engine
    e, rec = _gen().new_engine(engine)
    try:
        make = lambda n: np.zeros((n, 5), dtype=np.uint64)
        e.sc_muladd(make(3), make(3), make(3))
        assert len(rec.calls) == 1
        for short in range(1, 4):
            for n in (2, 4):
                rows = [make(n if i == short else 3) for i in range(4)]
                with pytest.raises(AssertionError):
                    e.sc_muladd(*rows[:3], **({"out": rows[3]} if short == 3 else {}))
        for bad in (np.zeros((3, 32), dtype=np.uint8), np.zeros((3, 5), dtype=np.uint64)):
            with pytest.raises(AssertionError):
                e.sc_from_bytes_wide(bad)                                                        # not 64 bytes per row
        assert len(rec.calls) == 1
    finally:
        e.ctx = None


def test_the_methods_live_on_a_base_class_of_engine():
    """The recorded method table of tests/test_engine_calls.py lists what `class Engine` itself defines; the four come from
    ScalarExtMixin."""
    from dusk_zerocaf_amd import engine, scalar_ext
    assert issubclass(engine.Engine, scalar_ext.ScalarExtMixin)
    for m in ("sc_from_bytes_wide", "sc_from_bytes_mod_order", "sc_muladd", "sc_invert"):
        assert m not in vars(engine.Engine) and callable(getattr(engine.Engine, m))


def test_cpp_and_rust_mirrors_and_documents():
    hpp = open(os.path.join(ROOT, "dusk_zerocaf_amd", "include", "zerocaf.hpp")).read()
    rs = open(os.path.join(ROOT, "integration", "rust", "zerocaf-hip", "src", "lib.rs")).read()
    ffi = open(os.path.join(ROOT, "integration", "rust", "zerocaf-hip", "src", "ffi.rs")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for s in SIGNATURES:
        assert s + "(" in hpp and "ffi::" + s + "(" in rs and "pub fn " + s + "(" in ffi and "pub fn " + s[3:] + "(" in rs, s
        assert s in integ and s in readme, s
    assert "92 entry points" in readme and "**all 92** entry points" in integ
    assert "k_sc_muladd" in design and "k_sc_invert_chunked" in design and "W256_RR" in design
