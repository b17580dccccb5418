"""CPU tier: the point sums (zc_ed_sum_rows, zc_ris_sum_rows) are declared with their contract in
include/zerocaf_hip_ext_sum_rows.h, which include/zerocaf_hip_ext.h includes on the line after zerocaf_hip_ext_gens.h; exported by
both libraries; bound in Python beside the 0.6 table and not inside it; refuse a missing pointer by name and in order, then the
context; reach the library from the Engine with the right symbol, argument order, shapes and dtypes.  (No GPU: the library calls
fail on their arguments, the Engine calls go to a recording stand-in, as in tests/test_engine_calls.py.)"""
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
SUM_HEADER = os.path.join(ROOT, "include", "zerocaf_hip_ext_sum_rows.h")
ED, RIS = "zc_ed_sum_rows", "zc_ris_sum_rows"
NAMES = [ED, RIS]
PROTOTYPES = ["int zc_ed_sum_rows (zc_ctx *ctx, const uint64_t *points, size_t terms, uint64_t *out, size_t n);",
              "int zc_ris_sum_rows(zc_ctx *ctx, const uint8_t *in32, size_t terms, uint8_t *out32, uint8_t *ok, size_t n);"]
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


def test_the_header_declares_exactly_the_two_prototypes_and_comes_in_after_the_gens_one():
    sh, ext, main = open(SUM_HEADER).read(), open(EXT_HEADER).read(), open(HEADER).read()
    decls = _squeeze(re.sub(r"/\*.*?\*/", "", sh, flags=re.S))
    for proto in PROTOTYPES:
        assert _squeeze(proto) in decls, proto
    assert _names(sh) == set(NAMES) and '#include "zerocaf_hip.h"' in sh
    outer = re.sub(r"/\*.*?\*/", "", ext, flags=re.S)
    assert re.search(r'^#include "zerocaf_hip_ext_gens.h"\n#include "zerocaf_hip_ext_sum_rows.h"\n', outer, flags=re.M)
    assert len(_names(ext)) == 1 and len(_names(main)) == 92
    assert len(_names(open(os.path.join(ROOT, "include", "zerocaf_hip_ext_sum.h")).read())) == 1
    for other in (main, ext):
        assert not any(name in other for name in NAMES)
    flat = " ".join(sh.replace("\n *", "\n").split()).lower()                     # the comment's text without its line prefixes
    for word in ("n * terms * 20 limbs", "row-major", "n * terms * 32 bytes", "not capped at 8", "2^24 points", "as zc_ed_add reads one", "src/edwards.rs:465-489",
                 "function of terms alone", "p = 1 for terms <= 32", "largest power of two with 16 * p <= terms", "at most 2^16", "s, s + p, s + 2 p",
                 "folded from the left", "adjacent pairs", "zc_ed_fold_ordered", "do not depend on n", "reduced mod p", "identity rows (0, 1, 1, 0)",
                 "pad with identity points", "deterministic garbage", "ok[i] = 0 and 32 zero bytes", "ok may be null", "32 zero bytes with ok = 1",
                 "no intermediate point", "null pointer: points", "null pointer: in32", "null pointer: out", "null pointer: out32", "null context", "2^31",
                 "n == 0: zc_ok", "zc_err_mixed_mem", "chunks of whole rows", "8-byte alignment", "must not overlap", "rows 0 .. n-1", "more than 8191 terms",
                 "no environment knob", "constant-time"):
        assert word in flat, word


@pytest.mark.parametrize("header", ["zerocaf_hip_ext.h", "zerocaf_hip_ext_sum_rows.h"])
def test_the_header_is_plain_c11(tmp_path, header):
    """Compiled as C11 with warnings as errors, alone and through the outer header; the prototypes are the ones a C caller links against."""
    src = tmp_path / "t.c"
    src.write_text('#include "%s"\n' % header +
                   "int (*const fe)(zc_ctx *, const uint64_t *, size_t, uint64_t *, size_t) = zc_ed_sum_rows;\n"
                   "int (*const fr)(zc_ctx *, const uint8_t *, size_t, uint8_t *, uint8_t *, size_t) = zc_ris_sum_rows;\n"
                   "int main(void) { return fe(0, 0, 3, 0, 0) == ZC_ERR_BAD_ARG && fr(0, 0, 3, 0, 0, 0) == ZC_ERR_BAD_ARG ? 0 : 1; }\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-c", "-o", str(tmp_path / "t.o"), str(src)])


def test_both_libraries_export_them_and_python_binds_them_beside_the_table(lib):
    import dusk_zerocaf_amd as z
    from dusk_zerocaf_amd import _lib
    for path in (z.LIB_PATH, _lib.TEST_LIB_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        assert set(NAMES) <= set(re.findall(r"\bT (zc_[a-z0-9_]+)", out)), path
        assert not [s for s in re.findall(r"\bT (zc_test_[a-z0-9_]+)", out) if "sum_rows" in s and "ris_sum_rows" not in s]
    v, n = C.c_void_p, C.c_size_t
    assert list(_lib.EXT_SUM_ROWS_SIGNATURES) == NAMES
    assert _lib.EXT_SUM_ROWS_SIGNATURES[ED] == [v, n, v, n] and _lib.EXT_SUM_ROWS_SIGNATURES[RIS] == [v, n, v, v, n]
    for name in NAMES:
        assert name not in z.ALL_SYMBOLS
        for table in (_lib.SIGNATURES, _lib.SCALAR_EXT_SIGNATURES, _lib.EXT_SIGNATURES, _lib.EXT_SUM_SIGNATURES, _lib.EXT_HASH_SIGNATURES, _lib.EXT_SHARED_SIGNATURES,
                      _lib.EXT_SHARED_LINCOMB_SIGNATURES, _lib.EXT_GENS_SIGNATURES):
            assert name not in table
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(_lib.EXT_SUM_ROWS_SIGNATURES[name]) + 1
    assert lib.zc_version().decode().startswith("zerocaf_hip 0.6 ")                  # additive: the ABI number stays


def test_refusals_come_by_name_and_in_order_before_the_context_is_touched(lib):
    """ctx = NULL throughout: a NULL pointer is named, the first in the header's order when both are missing, for n = 0 and for
    n * terms at the limit too; with both pointers in place the call gets as far as the context ("null context")."""
    p, out, e32, o32, ok = (np.zeros(60, dtype=np.uint64), np.zeros(40, dtype=np.uint64), np.zeros(96, dtype=np.uint8), np.zeros(64, dtype=np.uint8),
                            np.zeros(2, dtype=np.uint8))
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    err = lambda: lib.zc_last_error().decode()
    for terms in (0, 1, 3, 1 << 20, 1 << 40):
        for n in (1, 0, 1 << 31, 1 << 40):
            assert lib.zc_ed_sum_rows(None, ptr(p), terms, ptr(out), n) == ZC_ERR_BAD_ARG and err() == "null context"
            assert lib.zc_ed_sum_rows(None, None, terms, ptr(out), n) == ZC_ERR_BAD_ARG and err() == "null pointer: points"
            assert lib.zc_ed_sum_rows(None, ptr(p), terms, None, n) == ZC_ERR_BAD_ARG and err() == "null pointer: out"
            assert lib.zc_ed_sum_rows(None, None, terms, None, n) == ZC_ERR_BAD_ARG and err() == "null pointer: points"
            for okp in (ptr(ok), None):
                assert lib.zc_ris_sum_rows(None, ptr(e32), terms, ptr(o32), okp, n) == ZC_ERR_BAD_ARG and err() == "null context"
                assert lib.zc_ris_sum_rows(None, None, terms, ptr(o32), okp, n) == ZC_ERR_BAD_ARG and err() == "null pointer: in32"
                assert lib.zc_ris_sum_rows(None, ptr(e32), terms, None, okp, n) == ZC_ERR_BAD_ARG and err() == "null pointer: out32"
                assert lib.zc_ris_sum_rows(None, None, terms, None, okp, n) == ZC_ERR_BAD_ARG and err() == "null pointer: in32"
    assert not out.any() and not o32.any() and not ok.any() and not p.any() and not e32.any()
    src = open(os.path.join(ROOT, "dusk_zerocaf_amd", "csrc", "zerocaf_hip.hip")).read()
    body = src[src.index("static int sum_rows_args("):src.index("int zc_ed_sum_rows(")]
    assert body.index('"null context"') < body.index("n * terms must stay below 2^31")          # the context before the limit


@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_the_engine_methods_call_the_library_as_the_header_says(kind):
    """The symbol, then ctx, the rows, terms, the output(s), n; outputs of the input's kind."""
    from dusk_zerocaf_amd import engine
    n, terms = 3, 5
    e, rec = _gen().new_engine(engine)
    try:
        P = np.arange(n * terms * 20, dtype=np.uint64).reshape(n, terms, 20)
        E = (np.arange(n * terms * 32) % 251).astype(np.uint8).reshape(n, terms, 32)
        if kind == "torch":
            import torch
            P, E = torch.from_numpy(P.view(np.int64)), torch.from_numpy(E)
        ptr = lambda x: x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()
        got = e.ed_sum_rows(P)
        enc, ok = e.ris_sum_rows(E)
        with pytest.raises(AssertionError):
            e.ed_sum_rows(P.reshape(n * terms, 20))                                      # rows without a term dimension
        with pytest.raises(AssertionError):
            e.ris_sum_rows(E[:, :, :31])
        assert [c[0] for c in rec.calls] == [ED, RIS]
        a, b = rec.calls[0][1], rec.calls[1][1]
        assert a[0] is e.ctx and list(a[1:]) == [ptr(P), terms, ptr(got), n]
        assert b[0] is e.ctx and list(b[1:]) == [ptr(E), terms, ptr(enc), ptr(ok), n]
        assert tuple(got.shape) == (n, 20) and tuple(enc.shape) == (n, 32) and tuple(ok.shape) == (n,)
        assert "uint8" in str(enc.dtype) and "uint8" in str(ok.dtype) and "int64" in str(got.dtype)
        for x in (got, enc, ok):
            assert isinstance(x, np.ndarray) == (kind == "numpy")
        # rows without terms: nothing of the input is read, and the library still gets a pointer that is not NULL
        z = e.ed_sum_rows(P[:, :0])
        c = rec.calls[2][1]
        assert rec.calls[2][0] == ED and c[1] and list(c[2:]) == [0, ptr(z), n] and tuple(z.shape) == (n, 20)
    finally:
        e.ctx = None


def test_the_methods_live_on_a_base_class_of_engine():
    """The recorded method table of tests/test_engine_calls.py lists what `class Engine` itself defines."""
    from dusk_zerocaf_amd import engine, point_sums
    assert issubclass(engine.Engine, point_sums.PointSumsMixin)
    for m in ("ed_sum_rows", "ris_sum_rows"):
        assert m not in vars(engine.Engine) and m in vars(point_sums.PointSumsMixin) and callable(getattr(engine.Engine, m))


def test_cpp_and_rust_mirrors_and_documents():
    rd = lambda *parts: open(os.path.join(ROOT, *parts)).read()
    hpp = rd("dusk_zerocaf_amd", "include", "zerocaf.hpp")
    rust = os.path.join("integration", "rust", "zerocaf-hip", "src")
    ext_rs, lib_rs, ffi = rd(rust, "ext.rs"), rd(rust, "lib.rs"), rd(rust, "ffi.rs")
    readme, integ, design, exper = rd("README.md"), rd("INTEGRATION.md"), rd("DESIGN.md"), rd("DESIGN-EXPERIMENTS.md")
    assert "inline std::vector<EdwardsPoint> sum_rows(" in hpp and "inline std::vector<CompressedRistretto> sum_rows(" in hpp
    for name in NAMES:
        assert name + "(" in hpp and "pub fn " + name + "(" in ext_rs and "pub fn " + name[3:] + "(" in ext_rs
        assert name not in lib_rs and name not in ffi
        for doc in (readme, integ, design):
            assert name in doc, name
    for doc in (readme, integ, design):
        assert "zerocaf_hip_ext_sum_rows.h" in doc
    assert "92 entry points" in readme and "**all 92** entry points" in integ and "\n92 entry points (" in integ
    assert "### 4l" in integ
    worked = integ[integ.index("### 4l"):integ.index("## 5.")]
    for word in ("ElGamal tally", "key aggregation", "ris_sum_rows", "ed_sum_rows", "zerocaf::sum_rows", "EXT_SUM_ROWS_SIGNATURES", "point_sums.py"):
        assert word in worked, word
    assert "### 4.11" in design
    sec = design[design.index("### 4.11"):design.index("## 5.")]
    for word in ("zc_sum.hip.h", "zc_sum_plan.h", "Order of association", "16·P ≤ terms", "2¹⁶", "k_ed_rowsum", "k_ris_rowsum", "k_ed_rowsum_finish", "k_ris_rowsum_finish",
                 "VGPR", "LDS", "kernel_resources.py", "r21_sum_rows.json", "bench_sum_rows.py", "spread"):
        assert word in sec, word
    assert "round 21" in exper
    assert "r21_sum_rows.json" in readme and "tools/bench_sum_rows.py" in readme and "zc_sum.hip.h" in readme and "zc_sum_plan.h" in readme and "point_sums.py" in readme
    prof = __import__("json").load(open(os.path.join(ROOT, "profiles", "r21_sum_rows.json")))
    assert prof["tool"] == "tools/bench_sum_rows.py" and all(s["parity"] for s in prof["shapes"]) and len(prof["shapes"]) == 9
    from dusk_zerocaf_amd import build
    assert any(d.endswith("zerocaf_hip_ext_sum_rows.h") for d in build.DEPS) and "zc_sum.hip.h" in build.DEPS and "zc_sum_plan.h" in build.DEPS


def test_no_new_knob_hook_or_launch_plan_entry(lib):
    """`strings` of the product: the ZC_* knobs are the ten of tests/test_abi.py, none for these calls; zc_launch_plan.h does not
    know them."""
    import dusk_zerocaf_amd as z
    found = set(re.findall(rb"\x00(ZC_[A-Z][A-Z_0-9]+)(?=\x00)", open(z.LIB_PATH, "rb").read()))
    knobs = sorted(x.decode() for x in found if not x.startswith((b"ZC_ERR", b"ZC_OK")))
    assert knobs == ["ZC_HOST_CHUNKS", "ZC_INV_CHUNK", "ZC_JACOBI_ROUNDS", "ZC_MSM_AFFINE", "ZC_MSM_GROUPS", "ZC_MSM_WINDOW", "ZC_RCCL_PATH",
                     "ZC_RING_SLOTS", "ZC_RISTRETTO_STRICT", "ZC_SCHED"], knobs
    plan = open(os.path.join(ROOT, "dusk_zerocaf_amd", "csrc", "zc_launch_plan.h")).read()
    assert "rowsum" not in plan and "sum_rows" not in plan.replace("ris_sum_rows", "")
