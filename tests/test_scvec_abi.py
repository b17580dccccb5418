"""CPU tier: the scalar vector ops (zc_sc_sum_rows, zc_sc_dot_rows, zc_sc_powers) are declared with their contract in
include/zerocaf_hip_scvec.h -- a header of its own, plain C11, not a part of zerocaf_hip_ext.h; exported by both libraries; bound
in Python beside the 0.6 table and not inside it; refuse a missing pointer and a bad argument by name and in order, then the
context; reach the library from the Engine and from zerocaf_scvec.hpp with the right symbol, argument order, shapes and dtypes
(no GPU: the library calls fail on their arguments, the Engine and the C++ mirror go to recording stand-ins); are named by the
Rust shim and the documents; and profiles/r23_scvec.json is well-formed with parity true."""
import ctypes as C
import importlib.util
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HEADER = os.path.join(INC, "zerocaf_hip_scvec.h")
HPP = os.path.join(ROOT, "dusk_zerocaf_amd", "include", "zerocaf_scvec.hpp")
SUM, DOT, POW = "zc_sc_sum_rows", "zc_sc_dot_rows", "zc_sc_powers"
NAMES = [SUM, DOT, POW]
PROTOTYPES = ["int zc_sc_sum_rows(zc_ctx *ctx, const uint64_t *a, size_t terms, uint64_t *out, size_t n);",
              "int zc_sc_dot_rows(zc_ctx *ctx, const uint64_t *a, const uint64_t *b, size_t terms, unsigned flags, uint64_t *out, size_t n);",
              "int zc_sc_powers  (zc_ctx *ctx, const uint64_t *x, size_t terms, uint64_t *out, size_t n);"]
DLOG_NAMES = ["zc_dlog_create", "zc_dlog_destroy", "zc_ed_dlog", "zc_ris_dlog"]
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
    return re.sub(r"\s*\*\s*", " *", re.sub(r"\s*\(", "(", " ".join(text.split())))


def test_the_header_declares_exactly_the_three_prototypes_and_stands_alone():
    h = open(HEADER).read()
    decls = _squeeze(re.sub(r"/\*.*?\*/", "", h, flags=re.S))
    for proto in PROTOTYPES:
        assert _squeeze(proto) in decls, proto
    assert _names(h) == set(NAMES) and re.findall(r'#include\s+(\S+)', h) == ['"zerocaf_hip.h"']
    assert re.search(r"^#define ZC_SC_DOT_SHARED_B 1u(\s|$)", h, flags=re.M) and len(re.findall(r"^#define ZC_", h, flags=re.M)) == 1
    assert "zerocaf_hip_dlog.h" not in h and not any(name in h for name in DLOG_NAMES)
    # not one of the zerocaf_hip_ext* headers, not included by them, unknown to zerocaf_hip.h and zerocaf.hpp
    for f in os.listdir(INC):
        if f != "zerocaf_hip_scvec.h":
            other = open(os.path.join(INC, f)).read()
            assert "zerocaf_hip_scvec.h" not in other and not any(name in other for name in NAMES), f
    main = open(os.path.join(INC, "zerocaf_hip.h")).read()
    assert len(_names(main)) == 92
    hpp = open(os.path.join(ROOT, "dusk_zerocaf_amd", "include", "zerocaf.hpp")).read()
    assert "scvec" not in hpp.lower() and not any(name in hpp for name in NAMES)
    flat = " ".join(h.replace("\n *", "\n").split()).lower()                       # the comment's text without its line prefixes
    for word in ("by value", "zc_sc_muladd", "sum (w_i mod 2^52) 2^(52 i)", "260 bits", "canonical five limbs", "n * terms * 5 limbs", "row-major", "zc_ed_sum_rows",
                 "zc_sc_dot_shared_b", "one row of terms * 5 limbs", "unknown flag bits", "out[i][j] = val(x_i)^j", "out[i][0] = 1", "0 mod l", "not capped at 8", "2^24 terms",
                 "terms == 0 gives zero rows", "writes nothing", "associative", "null pointer: a", "null pointer: x", "null pointer: b", "null pointer: out", "null context",
                 "n * terms must stay below 2^31", "n == 0: zc_ok", "zc_err_mixed_mem", "chunks of whole rows", "synchronous", "each device once", "staging chunk",
                 "asynchronous on the context's stream", "8-byte alignment", "must not overlap", "rows 0 .. n-1", "no row changes another row's result", "workspace",
                 "different streams", "no environment knob", "constant-time"):
        assert word in flat, word


def test_the_header_is_plain_c11(tmp_path):
    """Compiled alone as C11 with warnings as errors and -pedantic; the prototypes are the ones a C caller links against."""
    src = tmp_path / "t.c"
    src.write_text('#include "zerocaf_hip_scvec.h"\n'
                   "int (*const fs)(zc_ctx *, const uint64_t *, size_t, uint64_t *, size_t) = zc_sc_sum_rows;\n"
                   "int (*const fd)(zc_ctx *, const uint64_t *, const uint64_t *, size_t, unsigned, uint64_t *, size_t) = zc_sc_dot_rows;\n"
                   "int (*const fp)(zc_ctx *, const uint64_t *, size_t, uint64_t *, size_t) = zc_sc_powers;\n"
                   "int main(void) { return fs(0, 0, 1, 0, 0) == ZC_ERR_BAD_ARG && fd(0, 0, 0, 1, ZC_SC_DOT_SHARED_B, 0, 0) == ZC_ERR_BAD_ARG && fp(0, 0, 1, 0, 0) == ZC_ERR_BAD_ARG ? 0 : 1; }\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + INC, "-c", "-o", str(tmp_path / "t.o"), str(src)])


def test_both_libraries_export_them_and_python_binds_them_beside_the_table(lib):
    import dusk_zerocaf_amd as z
    from dusk_zerocaf_amd import _lib
    for path in (z.LIB_PATH, _lib.TEST_LIB_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        assert set(NAMES) <= set(re.findall(r"\bT (zc_[a-z0-9_]+)", out)), path
        assert not [s for s in re.findall(r"\bT (zc_test_[a-z0-9_]+)", out) if "scvec" in s or "sc_dot" in s or "sc_powers" in s]
        assert "scvec_rows_launch" not in out and "scvec_args" not in out                # the host helpers stay internal
    v, n = C.c_void_p, C.c_size_t
    assert list(_lib.EXT_SCVEC_SIGNATURES) == NAMES
    assert _lib.EXT_SCVEC_SIGNATURES[SUM] == [v, n, v, n] == _lib.EXT_SCVEC_SIGNATURES[POW] and _lib.EXT_SCVEC_SIGNATURES[DOT] == [v, v, n, C.c_uint, v, n]
    for name in NAMES:
        assert name not in z.ALL_SYMBOLS
        for table in (_lib.SIGNATURES, _lib.SCALAR_EXT_SIGNATURES, _lib.EXT_SIGNATURES, _lib.EXT_SUM_SIGNATURES, _lib.EXT_HASH_SIGNATURES, _lib.EXT_SHARED_SIGNATURES,
                      _lib.EXT_SHARED_LINCOMB_SIGNATURES, _lib.EXT_GENS_SIGNATURES, _lib.EXT_SUM_ROWS_SIGNATURES, _lib.EXT_DLOG_SIGNATURES):
            assert name not in table
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(_lib.EXT_SCVEC_SIGNATURES[name]) + 1
    assert lib.zc_version().decode().startswith("zerocaf_hip 0.6 ")                  # additive: the ABI number stays


def test_refusals_come_by_name_and_in_order_before_the_context_is_touched(lib):
    """ctx = NULL throughout: a NULL pointer is named, the first in the header's order when several are missing, for n = 0 too and
    whatever terms; then the flag bits; with everything in place the call gets as far as the context ("null context")."""
    a, b, out = np.zeros(40, dtype=np.uint64), np.zeros(40, dtype=np.uint64), np.zeros(40, dtype=np.uint64)
    ptr = lambda x: None if x is None else C.c_void_p(x.ctypes.data)
    err = lambda: lib.zc_last_error().decode()
    for n in (1, 0, 1 << 31, 1 << 40):
        for terms in (0, 1, 8, 1 << 31, (1 << 64) - 1):
            for name, first in ((SUM, "a"), (POW, "x")):
                fn = getattr(lib, name)
                assert fn(None, ptr(a), terms, ptr(out), n) == ZC_ERR_BAD_ARG and err() == "null context"
                assert fn(None, None, terms, ptr(out), n) == ZC_ERR_BAD_ARG and err() == "null pointer: " + first
                assert fn(None, ptr(a), terms, None, n) == ZC_ERR_BAD_ARG and err() == "null pointer: out"
                assert fn(None, None, terms, None, n) == ZC_ERR_BAD_ARG and err() == "null pointer: " + first
            for flags in (0, 1):
                assert lib.zc_sc_dot_rows(None, ptr(a), ptr(b), terms, flags, ptr(out), n) == ZC_ERR_BAD_ARG and err() == "null context"
            for flags in (0, 1, 2, 1 << 31):                                          # the pointers before the flags
                assert lib.zc_sc_dot_rows(None, None, ptr(b), terms, flags, ptr(out), n) == ZC_ERR_BAD_ARG and err() == "null pointer: a"
                assert lib.zc_sc_dot_rows(None, ptr(a), None, terms, flags, ptr(out), n) == ZC_ERR_BAD_ARG and err() == "null pointer: b"
                assert lib.zc_sc_dot_rows(None, ptr(a), ptr(b), terms, flags, None, n) == ZC_ERR_BAD_ARG and err() == "null pointer: out"
                assert lib.zc_sc_dot_rows(None, None, None, terms, flags, None, n) == ZC_ERR_BAD_ARG and err() == "null pointer: a"
                assert lib.zc_sc_dot_rows(None, ptr(a), None, terms, flags, None, n) == ZC_ERR_BAD_ARG and err() == "null pointer: b"
            for flags in (2, 3, 4, 1 << 31, (1 << 32) - 2):                            # the flags before the context
                assert lib.zc_sc_dot_rows(None, ptr(a), ptr(b), terms, flags, ptr(out), n) == ZC_ERR_BAD_ARG and err() == "zc_sc_dot_rows: unknown flag bits"
    assert not a.any() and not b.any() and not out.any()


@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_the_engine_methods_call_the_library_as_the_header_says(kind):
    """The symbol, then ctx, the rows, terms, the flags, out, n; outputs of the input's kind and of the stated shape."""
    from dusk_zerocaf_amd import engine
    n, t = 3, 4
    e, rec = _gen().new_engine(engine)
    try:
        a = np.arange(n * t * 5, dtype=np.uint64).reshape(n, t, 5)
        b = a + np.uint64(7)
        row = np.arange(t * 5, dtype=np.uint64).reshape(t, 5)
        x = np.arange(n * 5, dtype=np.uint64).reshape(n, 5)
        if kind == "torch":
            import torch
            a, b, row, x = (torch.from_numpy(y.view(np.int64)) for y in (a, b, row, x))
        ptr = lambda y: y.ctypes.data if isinstance(y, np.ndarray) else y.data_ptr()
        s, d, ds, p = e.sc_sum_rows(a), e.sc_dot_rows(a, b), e.sc_dot_rows(a, row, shared_b=True), e.sc_powers(x, 6)
        with pytest.raises(AssertionError):
            e.sc_dot_rows(a, row)                                                       # one row where n rows belong
        with pytest.raises(AssertionError):
            e.sc_dot_rows(a, b, shared_b=True)
        with pytest.raises(AssertionError):
            e.sc_sum_rows(x)                                                            # no terms axis
        assert [c[0] for c in rec.calls] == [SUM, DOT, DOT, POW]
        c0, c1, c2, c3 = (c[1] for c in rec.calls)
        assert c0[0] is e.ctx and list(c0[1:]) == [ptr(a), t, ptr(s), n]
        assert c1[0] is e.ctx and list(c1[1:4]) == [ptr(a), ptr(b), t] and isinstance(c1[4], C.c_uint) and c1[4].value == 0 and list(c1[5:]) == [ptr(d), n]
        assert list(c2[1:4]) == [ptr(a), ptr(row), t] and isinstance(c2[4], C.c_uint) and c2[4].value == 1 and list(c2[5:]) == [ptr(ds), n]
        assert c3[0] is e.ctx and list(c3[1:]) == [ptr(x), 6, ptr(p), n]
        for res, shape in ((s, (n, 5)), (d, (n, 5)), (ds, (n, 5)), (p, (n, 6, 5))):
            assert tuple(res.shape) == shape and isinstance(res, np.ndarray) == (kind == "numpy") and ("uint64" in str(res.dtype) or "int64" in str(res.dtype))
        z = e.sc_sum_rows(a[:, :0])                                                     # terms = 0: nothing of a is read
        assert tuple(z.shape) == (n, 5) and rec.calls[-1][1][2] == 0 and rec.calls[-1][1][1] == rec.calls[-1][1][3] == ptr(z)
    finally:
        e.ctx = None


def test_the_methods_live_on_a_base_class_of_engine():
    """The recorded method table of tests/test_engine_calls.py lists what `class Engine` itself defines."""
    from dusk_zerocaf_amd import engine, scalar_vec
    assert issubclass(engine.Engine, scalar_vec.ScalarVecMixin) and scalar_vec.DOT_SHARED_B == 1
    for m in ("sc_sum_rows", "sc_dot_rows", "sc_powers"):
        assert m not in vars(engine.Engine) and m in vars(scalar_vec.ScalarVecMixin) and callable(getattr(engine.Engine, m))


# ------------------------------------------------------------------ zerocaf_scvec.hpp on a recording stand-in
DRIVER = r"""
#include <cstdio>
#include "zerocaf_scvec.hpp"
using namespace zerocaf;
static void show(const char* what, const std::vector<Scalar>& r)
{
    std::printf("%s", what);
    for (const auto& x : r) std::printf(" %llu", (unsigned long long)x.l[0]);
    std::printf("\n");
}
int main()
{
    std::vector<std::vector<Scalar>> a(3, std::vector<Scalar>(2)), b(3, std::vector<Scalar>(2));
    a[1][1] = Scalar(7);
    b[2][0] = Scalar(9);
    std::vector<Scalar> w = {Scalar(5), Scalar(6)}, x = {Scalar(3), Scalar(4)};
    show("sum", sc_sum_rows(a));
    show("dot", sc_dot_rows(a, b));
    show("shared", sc_dot_rows(a, w));
    const auto p = sc_powers(x, 3);
    std::printf("powers %zu %zu\n", p.size(), p[0].size());
    show("row", p[1]);
    show("none", sc_sum_rows({}));
    std::printf("empty %zu\n", sc_powers(x, 0)[1].size());
    try {
        a[2].pop_back();
        sc_sum_rows(a);
        std::printf("no exception\n");
    } catch (const std::invalid_argument& e) {
        std::printf("! %s\n", e.what());
    }
    return 0;
}
"""


def test_the_cpp_mirror_calls_the_library_as_the_header_says(tmp_path):
    """tests/cpp/mirror_standin.py, unchanged, with the three prototypes and their extents on top of the table of
    tests/test_cpp_mirror_calls.py: the logged calls and what the wrappers return from the stand-in's patterns."""
    from tests import test_cpp_mirror_calls as MC
    SI = MC.SI
    shapes = dict(MC.SHAPES)
    shapes.update({SUM: dict(a=SI.IN(8, "5 * terms * n"), out=SI.OUT(8, 5)),
                   DOT: dict(a=SI.IN(8, "5 * terms * n"), b=SI.IN(8, "(flags & 1) ? 5 * terms : 5 * terms * n"), out=SI.OUT(8, 5)),
                   POW: dict(x=SI.IN(8, "5 * n"), out=SI.OUT(8, "5 * terms"))})
    protos = MC.all_prototypes(open(HEADER).read())
    assert {n for n, _ in protos} >= set(NAMES)
    (tmp_path / "standin.cpp").write_text(SI.source(protos, shapes))
    so = str(tmp_path / "libzerocaf_hip.so")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-fPIC", "-shared", "-Wall", "-I" + INC, "-o", so, str(tmp_path / "standin.cpp")])
    (tmp_path / "driver.cpp").write_text(DRIVER)
    exe = str(tmp_path / "driver")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-Wall", "-Wextra", "-Werror", "-I" + os.path.dirname(HPP), str(tmp_path / "driver.cpp"), "-o", exe,
                           "-L" + str(tmp_path), "-lzerocaf_hip", "-Wl,-rpath," + str(tmp_path)])
    log = str(tmp_path / "calls.log")
    run = subprocess.run([exe], env=dict(os.environ, ZC_STANDIN_LOG=log, ZC_STANDIN_FAIL=""), capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr[-500:]
    sid = {n: i + 1 for i, n in enumerate(sorted(n for n, _ in protos))}
    pat = lambda sym, i, w=0: SI.pattern(sid[sym], 0, i, w, 8)
    lines = run.stdout.splitlines()
    assert lines[0] == "sum %d %d %d" % tuple(pat(SUM, i) for i in range(3)) and lines[1] == "dot %d %d %d" % tuple(pat(DOT, i) for i in range(3)) and lines[2].startswith("shared ")
    assert lines[3] == "powers 2 3" and lines[4] == "row %d %d %d" % tuple(pat(POW, 1, 5 * j) for j in range(3)) and lines[5:8] == ["none", "empty 0", "! sc_sum_rows: rows of different lengths"]
    calls = [l.split() for l in open(log).read().splitlines() if l.split()[0] in NAMES]
    hexw = lambda words: "".join(int(w).to_bytes(8, "little").hex() for w in words)
    sc = lambda v: [v, 0, 0, 0, 0]
    fa = sc(0) + sc(0) + sc(0) + sc(7) + sc(0) + sc(0)
    fb = sc(0) * 4 + sc(9) + sc(0)
    assert calls[0] == [SUM, "ctx=ok", "a=" + hexw(fa), "terms=2", "out=PTR", "n=3"]
    assert calls[1] == [DOT, "ctx=ok", "a=" + hexw(fa), "b=" + hexw(fb), "terms=2", "flags=0", "out=PTR", "n=3"]
    assert calls[2] == [DOT, "ctx=ok", "a=" + hexw(fa), "b=" + hexw(sc(5) + sc(6)), "terms=2", "flags=1", "out=PTR", "n=3"]
    assert calls[3] == [POW, "ctx=ok", "x=" + hexw(sc(3) + sc(4)), "terms=3", "out=PTR", "n=2"] and len(calls) == 4      # no call for no rows, for no terms, for ragged rows
    run = subprocess.run([exe], env=dict(os.environ, ZC_STANDIN_LOG=log, ZC_STANDIN_FAIL=DOT), capture_output=True, text=True, timeout=60)
    assert run.returncode != 0 or "zc_sc_dot_rows failed: " + SI.LAST_ERROR in run.stdout + run.stderr


def test_rust_mirror_and_documents():
    rd = lambda *parts: open(os.path.join(ROOT, *parts)).read()
    hpp, main_hpp = rd("dusk_zerocaf_amd", "include", "zerocaf_scvec.hpp"), rd("dusk_zerocaf_amd", "include", "zerocaf.hpp")
    rust = os.path.join("integration", "rust", "zerocaf-hip", "src")
    ext_rs, lib_rs, ffi = rd(rust, "ext.rs"), rd(rust, "lib.rs"), rd(rust, "ffi.rs")
    readme, integ, design, exper = rd("README.md"), rd("INTEGRATION.md"), rd("DESIGN.md"), rd("DESIGN-EXPERIMENTS.md")
    assert '#include "zerocaf.hpp"' in hpp and "zerocaf_hip_scvec.h" in hpp and "ZC_SC_DOT_SHARED_B" in hpp
    for name in NAMES:
        assert name + "(" in hpp and name not in main_hpp
        assert "pub fn " + name + "(" in ext_rs and "pub fn " + name[3:] + "(" in ext_rs
        assert name not in lib_rs and name not in ffi
        for doc in (readme, integ, design):
            assert name in doc, name
    assert "pub const ZC_SC_DOT_SHARED_B: u32 = 1;" in ext_rs and "pub fn sc_dot_rows_shared(" in ext_rs
    for doc in (readme, integ, design):
        assert "zerocaf_hip_scvec.h" in doc
    assert "92 entry points" in readme and "**all 92** entry points" in integ and "\n92 entry points (" in integ
    assert "### 4n" in integ
    worked = integ[integ.index("### 4n"):integ.index("## 5.")]
    for word in ("inner-product", "Shamir", DOT, POW, SUM, "zc_sc_muladd", "zc_ed_lincomb_shared", "ZC_SC_DOT_SHARED_B", "zerocaf_scvec.hpp", "shared_b=True"):
        assert word in worked, word
    assert "### 4.13" in design
    sec = design[design.index("### 4.13"):design.index("## 5. The oracle")]
    for word in ("zc_scvec.hip.h", "zc_scvec_plan.h", "k_sc_rowsum", "k_sc_rowdot", "k_sc_rowdot_part", "k_sc_rows_finish", "k_sc_powers", "SCV_CARRY_EVERY", "VGPR", "LDS",
                 "kernel_resources.py", "r23_scvec.json", "ZC_SCV_DOT_CHAINED", "slower"):
        assert word in sec, word
    assert "round 23" in exper.lower()
    assert "r23_scvec.json" in readme and "tools/bench_scvec.py" in readme and "zc_scvec.hip.h" in readme and "scalar_vec.py" in readme
    from dusk_zerocaf_amd import build
    assert any(d.endswith("zerocaf_hip_scvec.h") for d in build.DEPS) and "zc_scvec.hip.h" in build.DEPS and "zc_scvec_plan.h" in build.DEPS


def test_the_recorded_profile_is_well_formed_and_every_shape_agreed_with_its_compositions():
    with open(os.path.join(ROOT, "profiles", "r23_scvec.json")) as f:
        prof = json.load(f)
    assert prof["tool"] == "tools/bench_scvec.py" and prof["parity"] is True and prof["device"] and prof["ab_lib"]
    assert prof["sc_add"]["n"] == 1 << 24 and prof["sc_add"]["GB_per_s"] > 0
    got = [(s["call"], s["n"], s["terms"]) for s in prof["shapes"]]
    want = []
    for n, t in ((1 << 20, 2), (1 << 20, 8), (1 << 20, 64), (1, 1 << 20), (1, 1 << 24)):
        want += [("sc_dot_rows", n, t), ("sc_sum_rows", n, t)]
        if (n, t) == (1 << 20, 8):
            want.append(("sc_dot_rows_shared_b", n, t))
    want += [("sc_powers", 1 << 20, 8), ("sc_powers", 1, 1 << 24)]
    assert got == want
    for s in prof["shapes"]:
        assert s["parity"] is True and s["bytes_moved"] > 0 and s["over_bytes_bound"] > 0
        new = s["call"]
        assert new in s["paths"]
        for name, p in s["paths"].items():
            assert p["min_ms"] <= p["median_ms"] <= p["max_ms"] and len(p["samples_ms"]) in (prof["repeats"], prof["slow_repeats"])
            assert (name == new) == ("new_over_this" not in p)
        if s["call"] == "sc_dot_rows":
            assert "dot_chained_variant" in s["paths"] and (s["terms"] > 64 or "muladd_chain_presplit" in s["paths"])
            assert ("mul_download_host_sum" in s["paths"]) == (s["n"] * s["terms"] <= 1 << 21) == ("skipped" not in s)
        if s["call"] == "sc_sum_rows" and s["terms"] <= 64:
            assert "add_chain_presplit" in s["paths"]
        if s["call"] == "sc_powers" and s["terms"] <= 64:
            assert "pow_per_column" in s["paths"]
