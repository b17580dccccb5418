"""CPU tier: zc_ed_lincomb is declared, exported, callable from plain C and mirrored in Python, C++ and Rust.
(No GPU: every call here fails on its arguments before a device is touched.)"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zerocaf_hip.h")

SIGNATURE = ("int zc_ed_lincomb(zc_ctx *ctx, const uint64_t *points, const uint64_t *scalars, size_t terms, "
             "uint64_t *out, size_t n);")


@pytest.fixture(scope="module")
def lib():
    import dusk_zerocaf_amd as z
    if not os.path.exists(z.LIB_PATH):
        from dusk_zerocaf_amd import build
        build.build(test_hooks=True)
    return z.load()


def test_header_declares_the_entry_point():
    text = open(HEADER).read()
    decls = " ".join(re.sub(r"/\*.*?\*/", "", text, flags=re.S).split())
    assert " ".join(SIGNATURE.split()) in decls
    assert re.search(r"^#define ZC_LINCOMB_MAX_TERMS 8$", text, flags=re.M)


def test_library_exports_it(lib):
    import dusk_zerocaf_amd as z
    out = subprocess.check_output(["nm", "-D", "--defined-only", z.LIB_PATH], text=True)
    exported = set(re.findall(r"\bT (zc_[a-z0-9_]+)", out))
    assert "zc_ed_lincomb" in exported and "zc_ed_lincomb" in z.ALL_SYMBOLS
    assert lib.zc_version().decode().startswith("zerocaf_hip 0.6 ")                  # additive: the ABI number stays


def test_plain_c_caller_gets_bad_arg_without_a_context(lib, tmp_path):
    import dusk_zerocaf_amd as z
    src = tmp_path / "lincomb.c"
    src.write_text('''
#include "zerocaf_hip.h"
#include <stdio.h>
int main(void) {
    uint64_t pts[40] = {0}, k[10] = {0}, out[20];
    int (*lincomb)(zc_ctx *, const uint64_t *, const uint64_t *, size_t, uint64_t *, size_t) = zc_ed_lincomb;
    int a = lincomb(0, pts, k, 2, out, 1), b = lincomb(0, pts, k, ZC_LINCOMB_MAX_TERMS + 1, out, 1);
    printf("%d %d\\n", a, b);
    return a == ZC_ERR_BAD_ARG && b == ZC_ERR_BAD_ARG ? 0 : 1;
}
''')
    exe = tmp_path / "lincomb"
    libdir = os.path.dirname(z.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L", libdir, "-lzerocaf_hip", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib"])
    subprocess.check_call([str(exe)])


def test_engine_has_ed_lincomb():
    from dusk_zerocaf_amd.engine import Engine
    assert callable(getattr(Engine, "ed_lincomb", None))


def test_cpp_and_rust_mirrors_call_it():
    hpp = open(os.path.join(ROOT, "dusk_zerocaf_amd", "include", "zerocaf.hpp")).read()
    rs = open(os.path.join(ROOT, "integration", "rust", "zerocaf-hip", "src", "lib.rs")).read()
    ffi = open(os.path.join(ROOT, "integration", "rust", "zerocaf-hip", "src", "ffi.rs")).read()
    assert "zc_ed_lincomb(" in hpp and re.search(r"inline std::vector<EdwardsPoint> ed_lincomb\(", hpp)
    assert "ffi::zc_ed_lincomb(" in rs and "pub fn ed_lincomb(" in rs
    assert "pub fn zc_ed_lincomb(" in ffi


def test_documents_name_it():
    """README and INTEGRATION.md count 87 entry points and send 2..8 terms per row to zc_ed_lincomb (section 4c)."""
    readme = open(os.path.join(ROOT, "README.md")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "zc_ed_lincomb" in readme and "zc_ed_lincomb" in integ
    assert re.search(r"^#+ *4c\b", integ, flags=re.M)
