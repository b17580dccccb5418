"""CPU tier: zc_sha512_rows, zc_sc_from_sha512 and zc_ris_from_sha512 are declared with their contract in
include/zerocaf_hip_ext_hash.h, the part of the second public header (include/zerocaf_hip_ext.h, which includes it) for hashes
over batched rows; exported by both libraries, bound in Python in a table of their own, refuse their arguments in the header's
order before the context is touched, and reach the library from the Engine with the right symbol, argument order, pointer
arrays, shapes and dtypes.  (No GPU: the library calls fail on their arguments, the Engine calls go to a recording stand-in, as
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
HASH_HEADER = os.path.join(ROOT, "include", "zerocaf_hip_ext_hash.h")
MSG = "zc_ctx *ctx, const uint8_t *prefix, size_t prefix_len, const uint8_t *const *parts, const size_t *part_len, size_t nparts, "
PROTOTYPES = {
    "zc_sha512_rows": "int zc_sha512_rows(" + MSG + "uint8_t *out64, size_t n);",
    "zc_sc_from_sha512": "int zc_sc_from_sha512(" + MSG + "uint64_t *out, size_t n);",
    "zc_ris_from_sha512": "int zc_ris_from_sha512(" + MSG + "uint64_t *out, size_t n);",
}
NAMES = list(PROTOTYPES)
OUTS = {"zc_sha512_rows": ("out64", 64, np.uint8), "zc_sc_from_sha512": ("out", 5, np.uint64), "zc_ris_from_sha512": ("out", 20, np.uint64)}
METHODS = {"zc_sha512_rows": "sha512_rows", "zc_sc_from_sha512": "sc_from_sha512", "zc_ris_from_sha512": "ris_from_sha512"}
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


def test_the_hash_header_declares_the_three_with_their_contract_and_the_first_keeps_its_92_names():
    ext, main = open(HASH_HEADER).read(), open(HEADER).read()
    outer = re.sub(r"/\*.*?\*/", "", open(EXT_HEADER).read(), flags=re.S)
    assert re.search(r'^#include "zerocaf_hip_ext_sum.h"\n#include "zerocaf_hip_ext_hash.h"$', outer, flags=re.M) and '#include "zerocaf_hip.h"' in ext
    decls = " ".join(re.sub(r"/\*.*?\*/", "", ext, flags=re.S).split())
    for proto in PROTOTYPES.values():
        assert " ".join(proto.split()) in decls, proto
    assert _names(ext) == set(NAMES) and len(_names(main)) == 92 and not any(n in main for n in NAMES)
    assert len(_names(open(EXT_HEADER).read())) == 1 and len(_names(open(os.path.join(ROOT, "include", "zerocaf_hip_ext_sum.h")).read())) == 1
    for macro, value in (("ZC_HASH_MAX_PARTS", 4), ("ZC_HASH_MAX_PREFIX", 256), ("ZC_HASH_MAX_ROW_BYTES", 65535)):
        assert re.search(r"^#define %s\s+%d\b" % (macro, value), ext, flags=re.M), macro
    prose = " ".join(re.sub(r"^ \*( |$)", "", ext, flags=re.M).split())               # the comment's text without the line leaders
    flat = prose.lower()
    for word in ("FIPS 180-4", "zc_sc_from_bytes_wide", "zc_ris_from_uniform_bytes", "src/ristretto.rs:493-507", "little-endian 512-bit integer", "no digest reaches memory",
                 "always host memory", "null only when prefix_len == 0", "the stride equals the length", "null pointer: parts", "null pointer: part_len",
                 "null pointer: out64", "null pointer: out", "null pointer: prefix", "nparts outside 1 .. 4", "null pointer: parts[j]", "part_len[j] of 0",
                 "prefix_len > 256", "65535", "overflowing size_t", "null context", "n == 0", "ZC_ERR_MIXED_MEM", "synchronous", "asynchronous",
                 "no alignment", "an odd address", "8-byte alignment", "must not overlap", "nothing else", "no byte of any input", "no environment knob"):
        assert word.lower() in flat, word
    order = ["null pointer: parts\"", "null pointer: part_len", "null pointer: out64", "null pointer: prefix", "nparts outside", "null pointer: parts[j]",
             "part_len[j] of 0", "prefix_len > 256", "longer than 65535", "overflowing size_t", "null context"]
    at = [prose.index(w) for w in order]
    assert at == sorted(at), at


@pytest.mark.parametrize("header", ["zerocaf_hip_ext.h", "zerocaf_hip_ext_hash.h", "zerocaf_hip_ext_sum.h"])
def test_the_headers_are_plain_c11(tmp_path, header):
    """Compiled as C11 with warnings as errors through the second header and alone; the prototypes are the ones a C caller
    links against (the sum header alone does not bring the hash calls)."""
    src = tmp_path / "t.c"
    sig = "zc_ctx *, const uint8_t *, size_t, const uint8_t *const *, const size_t *, size_t, %s *, size_t"
    body = '#include "%s"\n' % header
    if header != "zerocaf_hip_ext_sum.h":
        body += "".join("int (*const f%d)(%s) = %s;\n" % (i, sig % ("uint8_t" if n == "zc_sha512_rows" else "uint64_t"), n) for i, n in enumerate(NAMES))
        body += "_Static_assert(ZC_HASH_MAX_PARTS == 4 && ZC_HASH_MAX_PREFIX == 256 && ZC_HASH_MAX_ROW_BYTES == 65535, \"limits\");\n"
        body += "int main(void) { return f0(0, 0, 0, 0, 0, 1, 0, 0) == ZC_ERR_BAD_ARG && f1(0, 0, 0, 0, 0, 1, 0, 0) == ZC_ERR_BAD_ARG && f2(0, 0, 0, 0, 0, 1, 0, 0) == ZC_ERR_BAD_ARG ? 0 : 1; }\n"
    else:
        body += "int main(void) { return 0; }\n"
    src.write_text(body)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-c", "-o", str(tmp_path / "t.o"), str(src)])


def test_both_libraries_export_them_and_python_binds_them_in_a_table_of_their_own(lib):
    import dusk_zerocaf_amd as z
    from dusk_zerocaf_amd import _lib
    for path in (z.LIB_PATH, _lib.TEST_LIB_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        assert set(NAMES) <= set(re.findall(r"\bT (zc_[a-z0-9_]+)", out)), path
    vp, sz = C.c_void_p, C.c_size_t
    assert list(_lib.EXT_HASH_SIGNATURES) == NAMES and all(_lib.EXT_HASH_SIGNATURES[n] == [vp, sz, vp, vp, sz, vp, sz] for n in NAMES)
    for n in NAMES:
        assert n not in z.ALL_SYMBOLS and not any(n in t for t in (_lib.SIGNATURES, _lib.SCALAR_EXT_SIGNATURES, _lib.EXT_SIGNATURES, _lib.EXT_SUM_SIGNATURES))
        fn = getattr(lib, n)
        assert fn.restype is C.c_int and len(fn.argtypes) == 8
    assert lib.zc_version().decode().startswith("zerocaf_hip 0.6 ")                  # additive: the ABI number stays


@pytest.mark.parametrize("name", NAMES)
def test_arguments_are_refused_in_order_before_the_context_is_touched(lib, name):
    """ctx = NULL throughout: with good arguments the call gets as far as the context ("null context"), for n = 0 too.  Each
    refusal of the header arrives with its message while everything LATER in the order is wrong as well.  Nothing is written."""
    out_name, width, dtype = OUTS[name]
    fn = getattr(lib, name)
    err = lambda: lib.zc_last_error().decode()
    a, b = np.zeros(64, dtype=np.uint8), np.zeros(64, dtype=np.uint8)
    out = np.full(4 * width, 0xA5, dtype=dtype)
    prefix = b"domain"
    P = lambda x: C.c_void_p(x.ctypes.data)
    ptrs = lambda *xs: (C.c_void_p * len(xs))(*[None if x is None else x.ctypes.data for x in xs])
    lens = lambda *ls: (C.c_size_t * len(ls))(*ls)
    huge = (1 << 64) - 1

    def call(prefix=prefix, prefix_len=6, parts=ptrs(a, b), part_len=lens(32, 32), nparts=2, o=P(out), n=2):
        return fn(None, prefix, prefix_len, parts, part_len, nparts, o, n), err()
    for n in (2, 0):
        assert call(n=n) == (ZC_ERR_BAD_ARG, "null context")
        assert call(prefix=None, prefix_len=0, n=n) == (ZC_ERR_BAD_ARG, "null context")      # no prefix
    # every later argument is bad too in each of these: the first in the header's order is the one reported
    bad_parts, bad_len = ptrs(None, None), lens(0, 70000)
    assert call(parts=None, part_len=None, o=None, prefix=None, nparts=9) == (ZC_ERR_BAD_ARG, "null pointer: parts")
    assert call(parts=bad_parts, part_len=None, o=None, prefix=None, nparts=9) == (ZC_ERR_BAD_ARG, "null pointer: part_len")
    assert call(parts=bad_parts, part_len=bad_len, o=None, prefix=None, nparts=9) == (ZC_ERR_BAD_ARG, "null pointer: %s" % out_name)
    assert call(parts=bad_parts, part_len=bad_len, prefix=None, prefix_len=300, nparts=9) == (ZC_ERR_BAD_ARG, "null pointer: prefix")
    for nparts in (0, 5, 9, huge):
        rc, msg = call(parts=bad_parts, part_len=bad_len, prefix_len=300, prefix=b"x" * 300, nparts=nparts)
        assert rc == ZC_ERR_BAD_ARG and "nparts must be 1 .. 4" in msg, msg
    assert call(parts=ptrs(a, None), part_len=bad_len, prefix_len=300, prefix=b"x" * 300) == (ZC_ERR_BAD_ARG, "null pointer: parts[1]")
    assert call(parts=bad_parts, part_len=bad_len, prefix_len=300, prefix=b"x" * 300) == (ZC_ERR_BAD_ARG, "null pointer: parts[0]")
    rc, msg = call(part_len=lens(32, 0), prefix_len=300, prefix=b"x" * 300, n=huge)
    assert rc == ZC_ERR_BAD_ARG and "part_len[1] must be at least 1" in msg, msg
    rc, msg = call(part_len=lens(70000, 32), prefix_len=257, prefix=b"x" * 257, n=huge)
    assert rc == ZC_ERR_BAD_ARG and "prefix_len must be at most 256" in msg, msg
    for pl, ls in ((6, (65535 - 6 - 32 + 1, 32)), (0, (65535, 1)), (256, (32, huge)), (0, (huge, huge)), (0, (1 << 63, 1 << 63))):
        rc, msg = call(part_len=lens(*ls), prefix_len=pl, prefix=b"x" * pl, n=huge)
        assert rc == ZC_ERR_BAD_ARG and "at most 65535 bytes" in msg, (pl, ls, msg)
    assert call(part_len=lens(65535 - 6 - 32, 32)) == (ZC_ERR_BAD_ARG, "null context")       # exactly at the limit
    assert call(prefix_len=256, prefix=b"x" * 256) == (ZC_ERR_BAD_ARG, "null context")
    # 2^59 rows of 32 bytes overflow; 2^59 - 1 rows fit the parts and overflow every one of the three outputs
    for n, refused in ((huge, True), (1 << 59, True), ((1 << 59) - 1, True), (1 << 40, False)):
        rc, msg = call(n=n)
        assert rc == ZC_ERR_BAD_ARG and (("overflow" in msg) == refused) and (refused or msg == "null context"), (n, msg)
    rc, msg = call(part_len=lens(32, 40000), n=(1 << 64) // 40000 + 1)
    assert rc == ZC_ERR_BAD_ARG and "n * part_len[1] overflows size_t" in msg, msg
    assert not a.any() and not b.any() and (out == 0xA5).all()


@pytest.mark.parametrize("kind", ["numpy", "torch"])
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("lens", [(7,), (32, 32, 32), (5, 3, 120, 1)], ids=lambda l: "x".join(map(str, l)))
def test_the_engine_methods_call_the_library_as_the_header_says(kind, name, lens):
    """One call: the symbol, then ctx, prefix (None when empty), prefix_len, an array of the parts' pointers, an array of their
    lengths as size_t, nparts, the output (of the parts' kind, the right shape and dtype), n."""
    from dusk_zerocaf_amd import engine
    n = 3
    out_name, width, dtype = OUTS[name]
    e, rec = _gen().new_engine(engine)
    try:
        conv = lambda a: a
        if kind == "torch":
            import torch
            conv = torch.from_numpy
        parts = [conv(((np.arange(n * l) + j) % 251).astype(np.uint8).reshape(n, l)) for j, l in enumerate(lens)]
        ptr = lambda x: x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()
        method = getattr(e, METHODS[name])
        for prefix in (b"", b"domain"):
            del rec.calls[:]
            got = method(parts, prefix) if prefix else method(parts)
            assert len(rec.calls) == 1 and rec.calls[0][0] == name
            args = rec.calls[0][1]
            assert len(args) == 8 and args[0] is e.ctx and args[1] == (prefix or None) and args[2] == len(prefix)
            assert isinstance(args[3], C.Array) and args[3]._type_ is C.c_void_p and list(args[3]) == [ptr(p) for p in parts]
            assert isinstance(args[4], C.Array) and args[4]._type_ is C.c_size_t and list(args[4]) == list(lens)
            assert args[5] == len(lens) and args[6] == ptr(got) and args[7] == n
            assert tuple(got.shape) == (n, width) and isinstance(got, np.ndarray) == (kind == "numpy")
            assert got.dtype == dtype if kind == "numpy" else got.element_size() == np.dtype(dtype).itemsize
        with pytest.raises(AssertionError):
            method(parts[:1] + [parts[0][:2]])                                            # row counts differ
        with pytest.raises(AssertionError):
            method([])
        with pytest.raises(AssertionError):
            method([parts[0]] * 5)                                                        # five parts
        with pytest.raises(AssertionError):
            method(parts, b"x" * 257)
        if kind == "torch":
            with pytest.raises(AssertionError):
                method([parts[0], np.zeros((n, 4), dtype=np.uint8)])                      # numpy beside tensors
        assert len(rec.calls) == 1
    finally:
        e.ctx = None


def test_the_methods_live_on_a_base_class_of_engine():
    """The recorded method table of tests/test_engine_calls.py lists what `class Engine` itself defines."""
    from dusk_zerocaf_amd import engine, hash_batch
    assert issubclass(engine.Engine, hash_batch.HashMixin)
    for m in METHODS.values():
        assert m not in vars(engine.Engine) and callable(getattr(engine.Engine, m))


def _rust_decl(text, name):
    m = re.search(r"pub fn %s\((.*?)\)\s*->\s*c_int;" % name, text, flags=re.S)
    assert m, name
    return [tuple(x.strip() for x in p.split(":")) for p in m.group(1).split(",")]


def test_the_rust_declarations_match_the_header():
    """Parameter for parameter: names, constness, pointee width."""
    rd = lambda *parts: open(os.path.join(ROOT, *parts)).read()
    rust = os.path.join("integration", "rust", "zerocaf-hip", "src")
    ext_rs, lib_rs, ffi = rd(rust, "ext.rs"), rd(rust, "lib.rs"), rd(rust, "ffi.rs")
    ctypes_to_rust = {"zc_ctx *": "*mut ZcCtx", "const uint8_t *const *": "*const *const u8", "const uint8_t *": "*const u8", "const size_t *": "*const usize",
                      "uint64_t *": "*mut u64", "uint8_t *": "*mut u8", "size_t ": "usize"}
    for name, proto in PROTOTYPES.items():
        params = re.search(r"%s\((.*?)\);" % name, " ".join(proto.split())).group(1).split(",")
        want = []
        for p in params:
            p = p.strip()
            nm = re.search(r"([a-z0-9_]+)$", p).group(1)
            want.append((nm, ctypes_to_rust[p[:len(p) - len(nm)]]))
        assert _rust_decl(ext_rs, name) == want
        assert "pub fn %s(" % METHODS[name] in ext_rs and name not in lib_rs and name not in ffi


def test_cpp_mirror_build_list_and_documents():
    rd = lambda *parts: open(os.path.join(ROOT, *parts)).read()
    hpp, build_py = rd("dusk_zerocaf_amd", "include", "zerocaf.hpp"), rd("dusk_zerocaf_amd", "build.py")
    readme, integ, design = rd("README.md"), rd("INTEGRATION.md"), rd("DESIGN.md")
    assert "zc_hash.hip.h" in build_py and "zerocaf_hip_ext_hash.h" in build_py
    from dusk_zerocaf_amd import build
    assert "zc_hash.hip.h" in build.DEPS and any(d.endswith("zerocaf_hip_ext_hash.h") for d in build.DEPS)      # the embedded source hash covers them
    for name in NAMES:
        assert name + "(" in hpp and METHODS[name] + "(" in hpp
        for doc in (readme, integ, design):
            assert name in doc, name
    for doc in (readme, integ, design):
        assert "zerocaf_hip_ext_hash.h" in doc
    assert "92 entry points" in readme and "tools/bench_hash.py" in readme and "profiles/r17_hash.json" in readme and "hash_batch.py" in readme and "zc_hash.hip.h" in readme
    assert re.search(r'zc_sc_from_sha512\(ctx, \(const uint8_t \*\)"domain", 6,', integ) and "4h" in integ
    for word in ("4.6", "k_sha512_rows", "k_sc_from_sha512", "k_ris_from_sha512", "word form", "byte form", "v_alignbit_b32", "scratch", "profiles/r17_hash.json"):
        assert word in design, word
    src = rd("dusk_zerocaf_amd", "csrc", "zerocaf_hip.hip")
    for name, kernel in zip(NAMES, ("k_sha512_rows", "k_sc_from_sha512", "k_ris_from_sha512")):
        body = src[src.index("int %s(" % name):]
        body = body[:body.index("\n}\n")]
        assert "hash_rows_call(ctx, zc::%s," % kernel in body, name
    helper = src[src.index("int hash_rows_call("):]
    helper = helper[:helper.index("\n}\n")]
    assert "run_batched(ctx, args, (int)nparts + 1, n," in helper and "}, false);" in helper and "hipLaunchKernelGGL(k," in helper
    strings = re.findall(r'"(ZC_[A-Z][A-Z_0-9]+)"', rd("dusk_zerocaf_amd", "csrc", "zc_hash.hip.h") + helper)
    assert strings == []                                                                  # no new environment knob
