"""CPU tier: the generator sets (zc_gens_create, zc_gens_destroy, zc_ed_mul_gens, zc_ris_mul_gens_compress) are declared with their
contract in include/zerocaf_hip_ext_gens.h, which include/zerocaf_hip_ext.h includes on the line after
zerocaf_hip_ext_shared_lincomb.h; exported by both libraries; bound in Python beside the 0.6 table and not inside it; refuse a
missing pointer by name and in order, then the context; reach the library from the Engine with the right symbol, argument
order, shapes and dtypes.  (No GPU: the library calls fail on their arguments, the Engine calls go to a recording stand-in, as
in tests/test_engine_calls.py.)"""
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
GENS_HEADER = os.path.join(ROOT, "include", "zerocaf_hip_ext_gens.h")
CREATE, DESTROY, ED, RIS = "zc_gens_create", "zc_gens_destroy", "zc_ed_mul_gens", "zc_ris_mul_gens_compress"
NAMES = [CREATE, DESTROY, ED, RIS]
PROTOTYPES = ["int zc_gens_create (zc_ctx *ctx, const uint64_t *points, size_t count, uint64_t *id_out);",
              "int zc_gens_destroy(zc_ctx *ctx, uint64_t id);",
              "int zc_ed_mul_gens (zc_ctx *ctx, uint64_t id, const uint64_t *scalars, uint64_t *out, size_t n);",
              "int zc_ris_mul_gens_compress(zc_ctx *ctx, uint64_t id, const uint64_t *scalars, uint8_t *out32, size_t n);"]
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


def _squeeze(text):
    return re.sub(r"\s*\(", "(", " ".join(text.split()))


def test_the_header_declares_exactly_the_four_prototypes_and_comes_in_after_the_shared_lincomb_one():
    gh, ext, main = open(GENS_HEADER).read(), open(EXT_HEADER).read(), open(HEADER).read()
    decls = _squeeze(re.sub(r"/\*.*?\*/", "", gh, flags=re.S))
    for proto in PROTOTYPES:
        assert _squeeze(proto) in decls, proto
    assert _names(gh) == set(NAMES) and '#include "zerocaf_hip.h"' in gh and re.search(r"^#define ZC_GENS_MAX 8$", gh, flags=re.M)
    outer = re.sub(r"/\*.*?\*/", "", ext, flags=re.S)
    assert re.search(r'^#include "zerocaf_hip_ext_shared.h"\n#include "zerocaf_hip_ext_shared_lincomb.h"\n#include "zerocaf_hip_ext_gens.h"\n', outer, flags=re.M)
    assert len(_names(ext)) == 1 and len(_names(main)) == 92
    for other in (main, ext):
        assert not any(name in other for name in NAMES)
    flat = " ".join(gh.replace("\n *", "\n").split()).lower()                     # the comment's text without its line prefixes
    for word in ("count * 20 limbs", "1 .. zc_gens_max", "t is ignored", "normalised to z = 1", "33 x 128", "540 kb", "every device slot", "synchronous",
                 "visible to any stream", "by value", "zero is decided by value", "generator %d is not a point of the curve", "*id_out is not written",
                 "the check runs on the device", "torsion and mixed-order points", "zc_msm_bases_create", "never reused", "unknown generator set",
                 "zc_ctx_destroy frees every live set", "row-major", "zc_ed_mul_base reads its scalar", "early-stop", "zc_scalar_mul_fast", "not by k mod l",
                 "32 zero bytes", "no ok output", "null pointer: scalars", "null pointer: out", "null pointer: out32", "null context", "2^31", "zc_err_mixed_mem",
                 "8-byte alignment", "rows 0 .. n-1", "no environment knob", "constant-time"):
        assert word in flat, word


@pytest.mark.parametrize("header", ["zerocaf_hip_ext.h", "zerocaf_hip_ext_gens.h"])
def test_the_header_is_plain_c11(tmp_path, header):
    """Compiled as C11 with warnings as errors, alone and through the outer header; the prototypes are the ones a C caller links against."""
    src = tmp_path / "t.c"
    src.write_text('#include "%s"\n' % header +
                   "int (*const fc)(zc_ctx *, const uint64_t *, size_t, uint64_t *) = zc_gens_create;\n"
                   "int (*const fd)(zc_ctx *, uint64_t) = zc_gens_destroy;\n"
                   "int (*const fe)(zc_ctx *, uint64_t, const uint64_t *, uint64_t *, size_t) = zc_ed_mul_gens;\n"
                   "int (*const fr)(zc_ctx *, uint64_t, const uint64_t *, uint8_t *, size_t) = zc_ris_mul_gens_compress;\n"
                   "int main(void) { return fc(0, 0, ZC_GENS_MAX, 0) == ZC_ERR_BAD_ARG && fd(0, 1) == ZC_ERR_BAD_ARG && fe(0, 1, 0, 0, 0) == ZC_ERR_BAD_ARG"
                   " && fr(0, 1, 0, 0, 0) == ZC_ERR_BAD_ARG ? 0 : 1; }\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-c", "-o", str(tmp_path / "t.o"), str(src)])


def test_both_libraries_export_them_and_python_binds_them_beside_the_table(lib):
    import dusk_zerocaf_amd as z
    from dusk_zerocaf_amd import _lib
    for path in (z.LIB_PATH, _lib.TEST_LIB_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        assert set(NAMES) <= set(re.findall(r"\bT (zc_[a-z0-9_]+)", out)), path
        assert not [s for s in re.findall(r"\bT (zc_test_[a-z0-9_]+)", out) if "gens" in s]
    v, n, u64 = C.c_void_p, C.c_size_t, C.c_uint64
    assert list(_lib.EXT_GENS_SIGNATURES) == NAMES
    assert _lib.EXT_GENS_SIGNATURES[CREATE] == [v, n, C.POINTER(u64)] and _lib.EXT_GENS_SIGNATURES[DESTROY] == [u64]
    assert _lib.EXT_GENS_SIGNATURES[ED] == [u64, v, v, n] and _lib.EXT_GENS_SIGNATURES[RIS] == [u64, v, v, n]
    for name in NAMES:
        assert name not in z.ALL_SYMBOLS
        for table in (_lib.SIGNATURES, _lib.SCALAR_EXT_SIGNATURES, _lib.EXT_SIGNATURES, _lib.EXT_SUM_SIGNATURES, _lib.EXT_HASH_SIGNATURES, _lib.EXT_SHARED_SIGNATURES,
                      _lib.EXT_SHARED_LINCOMB_SIGNATURES):
            assert name not in table
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(_lib.EXT_GENS_SIGNATURES[name]) + 1
    assert lib.zc_version().decode().startswith("zerocaf_hip 0.6 ")                  # additive: the ABI number stays


def test_refusals_come_by_name_and_in_order_before_the_context_is_touched(lib):
    """ctx = NULL throughout: a NULL pointer is named, the first in the header's order when both are missing, for n = 0 too and
    whatever the id; with both pointers in place the call gets as far as the context ("null context")."""
    k, out, o32 = np.zeros(40, dtype=np.uint64), np.zeros(40, dtype=np.uint64), np.zeros(64, dtype=np.uint8)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    err = lambda: lib.zc_last_error().decode()
    for name, o, oname in ((ED, out, "out"), (RIS, o32, "out32")):
        fn = getattr(lib, name)
        for n in (1, 0, 1 << 31, 1 << 40):
            for gid in (0, 1, 77):
                assert fn(None, gid, ptr(k), ptr(o), n) == ZC_ERR_BAD_ARG and err() == "null context"
                assert fn(None, gid, None, ptr(o), n) == ZC_ERR_BAD_ARG and err() == "null pointer: scalars"
                assert fn(None, gid, ptr(k), None, n) == ZC_ERR_BAD_ARG and err() == "null pointer: %s" % oname
                assert fn(None, gid, None, None, n) == ZC_ERR_BAD_ARG and err() == "null pointer: scalars"
    pts = np.zeros(160, dtype=np.uint64)
    gid = C.c_uint64(0xFEED)
    for count in (1, 8):
        assert lib.zc_gens_create(None, ptr(pts), count, C.byref(gid)) == ZC_ERR_BAD_ARG and err() == "null context"
        assert lib.zc_gens_create(None, None, count, C.byref(gid)) == ZC_ERR_BAD_ARG and err() == "null pointer: points"
        assert lib.zc_gens_create(None, ptr(pts), count, None) == ZC_ERR_BAD_ARG and err() == "null pointer: id_out"
    for count in (0, 9, 1 << 40):
        assert lib.zc_gens_create(None, ptr(pts), count, C.byref(gid)) == ZC_ERR_BAD_ARG and err() == "zc_gens_create: count must be 1 .. ZC_GENS_MAX"
    assert lib.zc_gens_destroy(None, 1) == ZC_ERR_BAD_ARG and err() == "null context"
    assert gid.value == 0xFEED and not out.any() and not o32.any() and not k.any()


class _Ids:
    """The recording stand-in, handing out a set id as the library would."""

    def __init__(self, rec):
        self._rec = rec

    def __getattr__(self, name):
        fn = getattr(self._rec, name)

        def wrapped(*args):
            if name == CREATE:
                args[-1]._obj.value = 91
            return fn(*args)
        return wrapped


@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_the_engine_methods_call_the_library_as_the_header_says(kind):
    """The symbol, then ctx, the id, the scalars, the output, n; outputs of the input's kind; the handle closes once."""
    from dusk_zerocaf_amd import engine, generators
    n, count = 3, 2
    e, rec = _gen().new_engine(engine)
    e.lib = _Ids(rec)
    try:
        pts = np.arange(count * 20, dtype=np.uint64).reshape(count, 20)
        K = np.arange(n * count * 5, dtype=np.uint64).reshape(n, count, 5)
        if kind == "torch":
            import torch
            pts, K = torch.from_numpy(pts.view(np.int64)), torch.from_numpy(K.view(np.int64))
        ptr = lambda x: x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()
        with e.generators(pts) as g:
            assert isinstance(g, generators.Generators) and (g.id, g.count) == (91, count)
            got = e.ed_mul_gens(g, K)
            enc = e.ris_mul_gens_compress(g, K)
            with pytest.raises(AssertionError):
                e.ed_mul_gens(g, K[:, :1])                                            # one scalar per row for two generators
            with pytest.raises(AssertionError):
                e.ris_mul_gens_compress(g, K.reshape(n * count, 5))                   # rows without a term dimension
        assert g.id == 0
        g.close()                                                                     # a second close is nothing
        with pytest.raises(Exception, match="closed"):
            e.ed_mul_gens(g, K)
        assert [c[0] for c in rec.calls] == [CREATE, ED, RIS, DESTROY]
        a = rec.calls[0][1]
        assert a[0] is e.ctx and a[1:3] == (ptr(pts), count) and type(a[3]).__name__ == "CArgObject" and isinstance(a[3]._obj, C.c_uint64)
        for call, res in ((rec.calls[1][1], got), (rec.calls[2][1], enc)):
            assert call[0] is e.ctx and isinstance(call[1], C.c_uint64) and call[1].value == 91 and list(call[2:]) == [ptr(K), ptr(res), n]
        d = rec.calls[3][1]
        assert d[0] is e.ctx and isinstance(d[1], C.c_uint64) and d[1].value == 91 and len(d) == 2
        assert tuple(got.shape) == (n, 20) and tuple(enc.shape) == (n, 32) and "uint8" in str(enc.dtype) and "int64" in str(got.dtype)
        for x in (got, enc):
            assert isinstance(x, np.ndarray) == (kind == "numpy")
    finally:
        e.ctx = None


def test_the_methods_live_on_a_base_class_of_engine():
    """The recorded method table of tests/test_engine_calls.py lists what `class Engine` itself defines."""
    from dusk_zerocaf_amd import engine, generators
    assert issubclass(engine.Engine, generators.GeneratorsMixin)
    for m in ("generators", "ed_mul_gens", "ris_mul_gens_compress"):
        assert m not in vars(engine.Engine) and m in vars(generators.GeneratorsMixin) and callable(getattr(engine.Engine, m))
    for m in ("close", "__enter__", "__exit__"):
        assert m in vars(generators.Generators)


def test_cpp_and_rust_mirrors_and_documents():
    rd = lambda *parts: open(os.path.join(ROOT, *parts)).read()
    hpp = rd("dusk_zerocaf_amd", "include", "zerocaf.hpp")
    rust = os.path.join("integration", "rust", "zerocaf-hip", "src")
    ext_rs, lib_rs, ffi = rd(rust, "ext.rs"), rd(rust, "lib.rs"), rd(rust, "ffi.rs")
    readme, integ, design = rd("README.md"), rd("INTEGRATION.md"), rd("DESIGN.md")
    for name in NAMES:
        assert name + "(" in hpp and "pub fn " + name + "(" in ext_rs and "pub fn " + name[3:] + "(" in ext_rs
        assert name not in lib_rs and name not in ffi
        for doc in (readme, integ, design):
            assert name in doc, name
    for doc in (readme, integ, design):
        assert "zerocaf_hip_ext_gens.h" in doc
    assert "92 entry points" in readme and "**all 92** entry points" in integ and "\n92 entry points (" in integ
    assert "### 4k" in integ
    worked = integ[integ.index("### 4k"):]
    for word in ("Pedersen", "compress(v·G + r·H)", "ElGamal", "(r·B, M + r·PK)", "zc_ed_add", ED, RIS, CREATE):
        assert word in worked, word
    assert "### 4.10" in design
    sec = design[design.index("### 4.10"):]
    for word in ("zc_gens.hip.h", "comb_table_column", "k_gens_table_build", "k_ed_mul_gens", "k_ris_mul_gens_compress", "VGPR", "LDS", "kernel_resources.py",
                 "4 MiB", "r20_gens.json", "231"):
        assert word in sec, word
    assert "r20_gens.json" in readme and "tools/bench_gens.py" in readme
    assert "zc_gens.hip.h" in readme and "generators.py" in readme
    from dusk_zerocaf_amd import build
    assert any(d.endswith("zerocaf_hip_ext_gens.h") for d in build.DEPS) and "zc_gens.hip.h" in build.DEPS      # the embedded source hash covers them


def test_no_new_knob_in_the_product(lib):
    """`strings` of the product: the ZC_* knobs are the ten of tests/test_abi.py, none for these calls."""
    import dusk_zerocaf_amd as z
    found = set(re.findall(rb"\x00(ZC_[A-Z][A-Z_0-9]+)(?=\x00)", open(z.LIB_PATH, "rb").read()))
    knobs = sorted(x.decode() for x in found if not x.startswith((b"ZC_ERR", b"ZC_OK")))
    assert knobs == ["ZC_HOST_CHUNKS", "ZC_INV_CHUNK", "ZC_JACOBI_ROUNDS", "ZC_MSM_AFFINE", "ZC_MSM_GROUPS", "ZC_MSM_WINDOW", "ZC_RCCL_PATH",
                     "ZC_RING_SLOTS", "ZC_RISTRETTO_STRICT", "ZC_SCHED"], knobs
