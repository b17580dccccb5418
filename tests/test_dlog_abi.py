"""CPU tier: the bounded discrete logs (zc_dlog_create, zc_dlog_destroy, zc_ed_dlog, zc_ris_dlog) are declared with their contract
in include/zerocaf_hip_dlog.h -- a header of its own, plain C11, not a part of zerocaf_hip_ext.h; exported by both libraries;
bound in Python beside the 0.6 table and not inside it; refuse a missing pointer and a bad argument by name and in order, then
the context; reach the library from the Engine and from zerocaf_dlog.hpp with the right symbol, argument order, shapes and
dtypes (no GPU: the library calls fail on their arguments, the Engine and the C++ mirror go to recording stand-ins); are named
by the Rust shim and the documents; and profiles/r22_dlog.json is well-formed with parity true."""
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
DLOG_HEADER = os.path.join(INC, "zerocaf_hip_dlog.h")
HPP = os.path.join(ROOT, "dusk_zerocaf_amd", "include", "zerocaf_dlog.hpp")
CREATE, DESTROY, ED, RIS = "zc_dlog_create", "zc_dlog_destroy", "zc_ed_dlog", "zc_ris_dlog"
NAMES = [CREATE, DESTROY, ED, RIS]
PROTOTYPES = ["int zc_dlog_create (zc_ctx *ctx, const uint64_t *point, unsigned table_bits, unsigned flags, uint64_t *id_out);",
              "int zc_dlog_destroy(zc_ctx *ctx, uint64_t id);",
              "int zc_ed_dlog (zc_ctx *ctx, uint64_t id, const uint64_t *p,    uint64_t bound, uint64_t *m_out, uint8_t *found, uint8_t *ok, size_t n);",
              "int zc_ris_dlog(zc_ctx *ctx, uint64_t id, const uint8_t  *in32, uint64_t bound, uint64_t *m_out, uint8_t *found, uint8_t *ok, size_t n);"]
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


def test_the_header_declares_exactly_the_four_prototypes_and_stands_alone():
    dh = open(DLOG_HEADER).read()
    decls = _squeeze(re.sub(r"/\*.*?\*/", "", dh, flags=re.S))
    for proto in PROTOTYPES:
        assert _squeeze(proto) in decls, proto
    assert _names(dh) == set(NAMES) and re.findall(r'#include\s+(\S+)', dh) == ['"zerocaf_hip.h"']
    for define in ("#define ZC_DLOG_MIN_BITS 4", "#define ZC_DLOG_MAX_BITS 22", "#define ZC_DLOG_MAX_STEPS 65536", "#define ZC_DLOG_COSET4 1u"):
        assert re.search("^" + re.escape(define) + r"(\s|$)", dh, flags=re.M), define
    # not one of the zerocaf_hip_ext* headers, not included by them, unknown to zerocaf_hip.h and zerocaf.hpp
    for f in os.listdir(INC):
        if f != "zerocaf_hip_dlog.h":
            other = open(os.path.join(INC, f)).read()
            assert "zerocaf_hip_dlog.h" not in other and not any(name in other for name in NAMES), f
    main = open(os.path.join(INC, "zerocaf_hip.h")).read()
    assert len(_names(main)) == 92
    hpp = open(os.path.join(ROOT, "dusk_zerocaf_amd", "include", "zerocaf.hpp")).read()
    assert "dlog" not in hpp.lower()
    flat = " ".join(dh.replace("\n *", "\n").split()).lower()                     # the comment's text without its line prefixes
    for word in ("20 limbs", "t is ignored", "4 * g with zc_dlog_coset4", "every device slot", "synchronously", "2^table_bits", "stride point", "64 launch offsets",
                 "null pointer: point", "null pointer: id_out", "table_bits must be zc_dlog_min_bits .. zc_dlog_max_bits", "unknown flag bits", "null context",
                 "not a point of the curve", "by value", "generator lies in e[8]", "multiple of l", "no two table entries coincide", "at most one m", "2^38",
                 "zc_msm_bases_create", "zc_gens_create", "never reused", "zc_ctx_destroy frees every live table", "unknown dlog table",
                 "found[i] = 1 and m_out[i] = m iff", "in e[4]", "found[i] = 0 and m_out[i] = 0", "bound is exact", "not reported", "ok may be null",
                 "changes no other row", "projective representative", "1024 giant steps", "launch 0 writes the not-found defaults", "context's stream",
                 "zc_ris_dlog needs a zc_dlog_coset4 table", "does not decode", "32 zero bytes", "null pointer: m_out", "null pointer: found", "n == 0: zc_ok",
                 "zc_err_mixed_mem", "8-byte alignment", "rows 0 .. n-1", "no environment knob", "constant-time"):
        assert word in flat, word


def test_the_header_is_plain_c11(tmp_path):
    """Compiled alone as C11 with warnings as errors and -pedantic; the prototypes are the ones a C caller links against."""
    src = tmp_path / "t.c"
    src.write_text('#include "zerocaf_hip_dlog.h"\n'
                   "int (*const fc)(zc_ctx *, const uint64_t *, unsigned, unsigned, uint64_t *) = zc_dlog_create;\n"
                   "int (*const fd)(zc_ctx *, uint64_t) = zc_dlog_destroy;\n"
                   "int (*const fe)(zc_ctx *, uint64_t, const uint64_t *, uint64_t, uint64_t *, uint8_t *, uint8_t *, size_t) = zc_ed_dlog;\n"
                   "int (*const fr)(zc_ctx *, uint64_t, const uint8_t *, uint64_t, uint64_t *, uint8_t *, uint8_t *, size_t) = zc_ris_dlog;\n"
                   "int main(void) { return fc(0, 0, ZC_DLOG_MIN_BITS, ZC_DLOG_COSET4, 0) == ZC_ERR_BAD_ARG && fd(0, 1) == ZC_ERR_BAD_ARG"
                   " && fe(0, 1, 0, (uint64_t)ZC_DLOG_MAX_STEPS << ZC_DLOG_MAX_BITS, 0, 0, 0, 0) == ZC_ERR_BAD_ARG && fr(0, 1, 0, 1, 0, 0, 0, 0) == ZC_ERR_BAD_ARG ? 0 : 1; }\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + INC, "-c", "-o", str(tmp_path / "t.o"), str(src)])


def test_both_libraries_export_them_and_python_binds_them_beside_the_table(lib):
    import dusk_zerocaf_amd as z
    from dusk_zerocaf_amd import _lib
    for path in (z.LIB_PATH, _lib.TEST_LIB_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        assert set(NAMES) <= set(re.findall(r"\bT (zc_[a-z0-9_]+)", out)), path
        assert not [s for s in re.findall(r"\bT (zc_test_[a-z0-9_]+)", out) if "dlog" in s]
    v, n, u64, u = C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint
    assert list(_lib.EXT_DLOG_SIGNATURES) == NAMES
    assert _lib.EXT_DLOG_SIGNATURES[CREATE] == [v, u, u, C.POINTER(u64)] and _lib.EXT_DLOG_SIGNATURES[DESTROY] == [u64]
    assert _lib.EXT_DLOG_SIGNATURES[ED] == [u64, v, u64, v, v, v, n] == _lib.EXT_DLOG_SIGNATURES[RIS]
    for name in NAMES:
        assert name not in z.ALL_SYMBOLS
        for table in (_lib.SIGNATURES, _lib.SCALAR_EXT_SIGNATURES, _lib.EXT_SIGNATURES, _lib.EXT_SUM_SIGNATURES, _lib.EXT_HASH_SIGNATURES, _lib.EXT_SHARED_SIGNATURES,
                      _lib.EXT_SHARED_LINCOMB_SIGNATURES, _lib.EXT_GENS_SIGNATURES, _lib.EXT_SUM_ROWS_SIGNATURES):
            assert name not in table
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(_lib.EXT_DLOG_SIGNATURES[name]) + 1
    assert lib.zc_version().decode().startswith("zerocaf_hip 0.6 ")                  # additive: the ABI number stays


def test_refusals_come_by_name_and_in_order_before_the_context_is_touched(lib):
    """ctx = NULL throughout: a NULL pointer is named, the first in the header's order when several are missing, for n = 0 too
    and whatever the id and the bound; with the pointers in place the call gets as far as the context ("null context")."""
    p, e, m, f, ok = np.zeros(40, dtype=np.uint64), np.zeros(64, dtype=np.uint8), np.zeros(2, dtype=np.uint64), np.zeros(2, dtype=np.uint8), np.zeros(2, dtype=np.uint8)
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    err = lambda: lib.zc_last_error().decode()
    for name, rows, rname in ((ED, p, "p"), (RIS, e, "in32")):
        fn = getattr(lib, name)
        for n in (1, 0, 1 << 31, 1 << 40):
            for tid in (0, 1, 77):
                for bound in (0, 1, 1 << 20, (1 << 64) - 1):
                    for okp in (ok, None):
                        assert fn(None, tid, ptr(rows), bound, ptr(m), ptr(f), ptr(okp), n) == ZC_ERR_BAD_ARG and err() == "null context"
                        assert fn(None, tid, None, bound, ptr(m), ptr(f), ptr(okp), n) == ZC_ERR_BAD_ARG and err() == "null pointer: %s" % rname
                        assert fn(None, tid, ptr(rows), bound, None, ptr(f), ptr(okp), n) == ZC_ERR_BAD_ARG and err() == "null pointer: m_out"
                        assert fn(None, tid, ptr(rows), bound, ptr(m), None, ptr(okp), n) == ZC_ERR_BAD_ARG and err() == "null pointer: found"
                        assert fn(None, tid, None, bound, None, None, ptr(okp), n) == ZC_ERR_BAD_ARG and err() == "null pointer: %s" % rname
                        assert fn(None, tid, ptr(rows), bound, None, None, ptr(okp), n) == ZC_ERR_BAD_ARG and err() == "null pointer: m_out"
    tid = C.c_uint64(0xFEED)
    bits_msg, flag_msg = "zc_dlog_create: table_bits must be ZC_DLOG_MIN_BITS .. ZC_DLOG_MAX_BITS", "zc_dlog_create: unknown flag bits"
    for bits in (4, 9, 22):
        for flags in (0, 1):
            assert lib.zc_dlog_create(None, ptr(p), bits, flags, C.byref(tid)) == ZC_ERR_BAD_ARG and err() == "null context"
            assert lib.zc_dlog_create(None, None, bits, flags, C.byref(tid)) == ZC_ERR_BAD_ARG and err() == "null pointer: point"
            assert lib.zc_dlog_create(None, ptr(p), bits, flags, None) == ZC_ERR_BAD_ARG and err() == "null pointer: id_out"
            assert lib.zc_dlog_create(None, None, bits, flags, None) == ZC_ERR_BAD_ARG and err() == "null pointer: point"
        for flags in (2, 3, 4, 1 << 31):
            assert lib.zc_dlog_create(None, ptr(p), bits, flags, C.byref(tid)) == ZC_ERR_BAD_ARG and err() == flag_msg
    for bits in (0, 3, 23, 64, (1 << 32) - 1):
        for flags in (0, 1, 2):                                                       # the table size before the flags
            assert lib.zc_dlog_create(None, ptr(p), bits, flags, C.byref(tid)) == ZC_ERR_BAD_ARG and err() == bits_msg
        assert lib.zc_dlog_create(None, None, bits, 2, C.byref(tid)) == ZC_ERR_BAD_ARG and err() == "null pointer: point"      # the pointers before both
    assert lib.zc_dlog_destroy(None, 1) == ZC_ERR_BAD_ARG and err() == "null context"
    assert tid.value == 0xFEED and not p.any() and not m.any() and not f.any() and not ok.any()


class _Ids:
    """The recording stand-in, handing out a table id as the library would."""

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
    """The symbol, then ctx, the id, the rows, the bound, m_out, found, ok, n; outputs of the input's kind; the handle closes once."""
    from dusk_zerocaf_amd import dlog, engine
    n = 3
    e, rec = _gen().new_engine(engine)
    e.lib = _Ids(rec)
    try:
        G = np.arange(20, dtype=np.uint64)
        pts = np.arange(n * 20, dtype=np.uint64).reshape(n, 20)
        enc = np.arange(n * 32, dtype=np.uint8).reshape(n, 32)
        if kind == "torch":
            import torch
            G, pts, enc = torch.from_numpy(G.view(np.int64)).reshape(1, 20), torch.from_numpy(pts.view(np.int64)), torch.from_numpy(enc)
        ptr = lambda x: x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()
        with e.dlog_table(G, 9, coset4=True) as tb:
            assert isinstance(tb, dlog.DlogTable) and (tb.id, tb.bits, tb.coset4) == (91, 9, True)
            got = tb.ed(pts, 1000)
            wire = tb.ris(enc, 77)
            with pytest.raises(AssertionError):
                tb.ed(enc, 5)                                                         # rows of 32 bytes where limbs belong
        assert tb.id == 0
        tb.close()                                                                    # a second close is nothing
        with pytest.raises(Exception, match="closed"):
            tb.ed(pts, 5)
        assert [c[0] for c in rec.calls] == [CREATE, ED, RIS, DESTROY]
        a = rec.calls[0][1]
        assert a[0] is e.ctx and a[1] == ptr(G) and (a[2].value, a[3].value) == (9, 1) and type(a[4]).__name__ == "CArgObject" and isinstance(a[4]._obj, C.c_uint64)
        for call, rows, bound, res in ((rec.calls[1][1], pts, 1000, got), (rec.calls[2][1], enc, 77, wire)):
            assert call[0] is e.ctx and isinstance(call[1], C.c_uint64) and call[1].value == 91 and call[2] == ptr(rows)
            assert isinstance(call[3], C.c_uint64) and call[3].value == bound and list(call[4:]) == [ptr(res[0]), ptr(res[1]), ptr(res[2]), n]
        d = rec.calls[3][1]
        assert d[0] is e.ctx and isinstance(d[1], C.c_uint64) and d[1].value == 91 and len(d) == 2
        for res in (got, wire):
            m, found, ok = res
            assert tuple(m.shape) == tuple(found.shape) == tuple(ok.shape) == (n,) and "int64" in str(m.dtype) and "uint8" in str(found.dtype) and "uint8" in str(ok.dtype)
            assert all(isinstance(x, np.ndarray) == (kind == "numpy") for x in res)
        plain = e.dlog_table(np.arange(20, dtype=np.uint64), 4)                       # a bare row of 20 limbs, no flag
        assert rec.calls[-1][0] == CREATE and (rec.calls[-1][1][2].value, rec.calls[-1][1][3].value) == (4, 0)
        plain.id = 0
    finally:
        e.ctx = None


def test_the_methods_live_on_a_base_class_of_engine():
    """The recorded method table of tests/test_engine_calls.py lists what `class Engine` itself defines."""
    from dusk_zerocaf_amd import dlog, engine
    assert issubclass(engine.Engine, dlog.DlogMixin)
    assert "dlog_table" not in vars(engine.Engine) and "dlog_table" in vars(dlog.DlogMixin) and callable(engine.Engine.dlog_table)
    for m in ("ed", "ris", "close", "__enter__", "__exit__"):
        assert m in vars(dlog.DlogTable)
    assert (dlog.MIN_BITS, dlog.MAX_BITS, dlog.MAX_STEPS, dlog.COSET4) == (4, 22, 65536, 1)


# ------------------------------------------------------------------ zerocaf_dlog.hpp on a recording stand-in
DRIVER = r"""
#include <cstdio>
#include "zerocaf_dlog.hpp"
using namespace zerocaf;
static void show(const char* what, const std::vector<std::optional<uint64_t>>& r)
{
    std::printf("%s", what);
    for (const auto& x : r) x ? std::printf(" %llu", (unsigned long long)*x) : std::printf(" -");
    std::printf("\n");
}
int main()
{
    EdwardsPoint g = EdwardsPoint::identity();
    g.X.l[0] = 7;
    std::vector<EdwardsPoint> ps(3, g);
    ps[1].Y.l[2] = 9;
    std::vector<CompressedRistretto> es(2);
    es[1].bytes[31] = 0x5a;
    {
        DlogTable a(g, 9), b(ps[1], 12, true);
        show("ed", a.ed(ps, 1000));
        show("ris", b.ris(es, 77));
        show("none", a.ed({}, 5));
        DlogTable c(std::move(a));
        a = std::move(b);
        std::printf("bits %u %u coset4 %d %d\n", a.bits(), c.bits(), (int)a.coset4(), (int)c.coset4());
    }
    try {
        DlogTable bad(g, 4);
        std::printf("no exception\n");
    } catch (const std::runtime_error& e) {
        std::printf("! %s\n", e.what());
    }
    return 0;
}
"""


def test_the_cpp_mirror_calls_the_library_as_the_header_says(tmp_path):
    """tests/cpp/mirror_standin.py, unchanged, with the four prototypes and their extents on top of the table of
    tests/test_cpp_mirror_calls.py: the logged calls, what the wrappers return from the stand-in's patterns, the destruction of
    moved tables (once each, by the owner), and the exception of a failing status."""
    from tests import test_cpp_mirror_calls as MC
    SI = MC.SI
    shapes = dict(MC.SHAPES)
    shapes.update({CREATE: dict(point=SI.IN(8, "20"), id_out=SI.IDOUT("table_bits")),
                   ED: dict(p=SI.IN(8, "20 * n"), m_out=SI.OUT(8, 1), found=SI.MASK(), ok=SI.MASK()),
                   RIS: dict(in32=SI.IN(1, "32 * n"), m_out=SI.OUT(8, 1), found=SI.MASK(), ok=SI.MASK())})
    protos = MC.all_prototypes(open(DLOG_HEADER).read())
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
    m = lambda sym, i: SI.pattern(sid[sym], 0, i, 0, 8)
    # found = 1, 0, 1, ...: the rows the wrappers keep
    assert run.stdout.splitlines()[:4] == ["ed %d - %d" % (m(ED, 0), m(ED, 2)), "ris %d -" % m(RIS, 0), "none", "bits 12 9 coset4 1 0"]
    calls = [l.split() for l in open(log).read().splitlines() if l.split()[0] in NAMES]
    hexw = lambda words: "".join(int(w).to_bytes(8, "little").hex() for w in words)
    g = [7, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    g1 = list(g)
    g1[7] = 9
    first, second = SI.FIRST_ID, SI.FIRST_ID + 1
    assert calls[0] == [CREATE, "ctx=ok", "point=" + hexw(g), "table_bits=9", "flags=0", "id_out=PTR"]
    assert calls[1] == [CREATE, "ctx=ok", "point=" + hexw(g1), "table_bits=12", "flags=1", "id_out=PTR"]
    assert calls[2] == [ED, "ctx=ok", "id=%d" % first, "p=" + hexw(g + g1 + g), "bound=1000", "m_out=PTR", "found=PTR", "ok=NULL", "n=3"]
    assert calls[3] == [RIS, "ctx=ok", "id=%d" % second, "in32=" + "00" * 63 + "5a", "bound=77", "m_out=PTR", "found=PTR", "ok=NULL", "n=2"]
    # no call for no rows; a = move(b) frees a's own table (already moved to c: nothing), then the scope frees c's (first) and a's (second)
    assert sorted(calls[4:6]) == sorted([[DESTROY, "ctx=ok", "id=%d" % first], [DESTROY, "ctx=ok", "id=%d" % second]]) and len(calls) == 8
    assert calls[6][:1] == [CREATE] and calls[7] == [DESTROY, "ctx=ok", "id=%d" % (SI.FIRST_ID + 2)] and run.stdout.splitlines()[4] == "no exception"
    run = subprocess.run([exe], env=dict(os.environ, ZC_STANDIN_LOG=log, ZC_STANDIN_FAIL=ED), capture_output=True, text=True, timeout=60)
    assert run.returncode != 0 or "zc_ed_dlog failed: " + SI.LAST_ERROR in run.stdout + run.stderr


def test_rust_mirror_and_documents():
    rd = lambda *parts: open(os.path.join(ROOT, *parts)).read()
    hpp, main_hpp = rd("dusk_zerocaf_amd", "include", "zerocaf_dlog.hpp"), rd("dusk_zerocaf_amd", "include", "zerocaf.hpp")
    rust = os.path.join("integration", "rust", "zerocaf-hip", "src")
    ext_rs, lib_rs, ffi = rd(rust, "ext.rs"), rd(rust, "lib.rs"), rd(rust, "ffi.rs")
    readme, integ, design, exper = rd("README.md"), rd("INTEGRATION.md"), rd("DESIGN.md"), rd("DESIGN-EXPERIMENTS.md")
    assert '#include "zerocaf.hpp"' in hpp and "class DlogTable" in hpp and "DlogTable(const DlogTable&) = delete;" in hpp and "DlogTable(DlogTable&& o) noexcept" in hpp
    for name in NAMES:
        assert name + "(" in hpp and name not in main_hpp
        assert "pub fn " + name + "(" in ext_rs and "pub fn " + name[3:] + "(" in ext_rs
        assert name not in lib_rs and name not in ffi
        for doc in (readme, integ, design):
            assert name in doc, name
    for doc in (readme, integ, design):
        assert "zerocaf_hip_dlog.h" in doc
    assert "92 entry points" in readme and "**all 92** entry points" in integ and "\n92 entry points (" in integ
    assert "### 4m" in integ
    worked = integ[integ.index("### 4m"):]
    for word in ("ElGamal", "tally", "zc_ris_sum_rows", "zc_ris_lincomb_shared", RIS, CREATE, "ZC_DLOG_COSET4", "zerocaf_dlog.hpp"):
        assert word in worked, word
    code = worked[worked.index("```python"):]
    code = code[:code.index("```", 10)]
    assert code.index("zc_ris_sum_rows") < code.index("zc_ris_lincomb_shared") < code.index("zc_ris_dlog")      # the pipeline, end to end
    assert "### 4.12" in design
    sec = design[design.index("### 4.12"):]
    for word in ("zc_dlog.hip.h", "zc_dlog_plan.h", "k_dlog_setup", "k_dlog_records", "k_ed_dlog", "k_ris_dlog", "DLOG_CHUNK", "VGPR", "LDS", "kernel_resources.py",
                 "r22_dlog.json", "E[8]"):
        assert word in sec, word
    assert "round 22" in exper.lower()
    assert "r22_dlog.json" in readme and "tools/bench_dlog.py" in readme and "zc_dlog.hip.h" in readme and "dlog.py" in readme
    from dusk_zerocaf_amd import build
    assert any(d.endswith("zerocaf_hip_dlog.h") for d in build.DEPS) and "zc_dlog.hip.h" in build.DEPS and "zc_dlog_plan.h" in build.DEPS


def test_the_recorded_profile_is_well_formed_and_every_shape_found_its_planted_m():
    with open(os.path.join(ROOT, "profiles", "r22_dlog.json")) as f:
        prof = json.load(f)
    assert prof["tool"] == "tools/bench_dlog.py" and prof["parity"] is True and prof["device"]
    text = open(os.path.join(ROOT, "dusk_zerocaf_amd", "csrc", "zc_dlog_plan.h")).read()
    assert prof["dlog_chunk"] == int(re.search(r"^#define ZC_DLOG_CHUNK (\d+)$", text, flags=re.M).group(1)) and prof["multiplications_per_step_by_count"] == 11
    assert [c["table_bits"] for c in prof["create"]] == [16, 20, 22]
    for c in prof["create"]:
        assert set(c["paths"]) == {"plain", "coset4"} and all(p["median_ms"] > 0 and p["spread"] >= 0 and len(p["samples_ms"]) == prof["repeats"] for p in c["paths"].values())
    assert [(s["table_bits"], s["bound_log2"], s["n"]) for s in prof["shapes"]] == [(16, 24, 1 << 20), (20, 32, 1 << 16), (22, 32, 1 << 18)]
    for s in prof["shapes"]:
        assert set(s["paths"]) == {"ed_random", "ed_worst", "ris_random", "ris_worst"} == set(s["parity"]) and all(s["parity"].values())
        assert s["giant_steps"] == 1 << (s["bound_log2"] - s["table_bits"]) and s["launches"] == -(-s["giant_steps"] // 1024)
        for p in s["paths"].values():
            assert p["min_ms"] <= p["median_ms"] <= p["max_ms"] and len(p["samples_ms"]) == prof["repeats"]
        assert 0 < s["paths"]["ed_worst"]["roof_fraction"] < 1
    ab = prof["chunk_ab"]                                                             # the product against a build with another DLOG_CHUNK, alternated
    assert ab["parity"] is True and ab["product_chunk"] == prof["dlog_chunk"] != ab["variant_chunk"]
    assert {k.split("_", 1)[0] for k in ab["paths"]} == {"chunk%d" % ab["product_chunk"], "chunk%d" % ab["variant_chunk"]}
    comp = prof["composition"]
    assert (comp["table_bits"], comp["bound_log2"], comp["n"]) == (16, 20, 1 << 16) and comp["parity"] is True
    assert set(comp["paths"]) == {"ed_dlog", "add_to_affine_download_numpy_lookup"} and comp["paths"]["ed_dlog"]["over_composition"] > 0
