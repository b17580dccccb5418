"""CPU tier: zc_ris_lincomb is declared, exported, callable from plain C and mirrored in Python, C++ and Rust.
(No GPU: every call here fails on its arguments before a device is touched.)"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zerocaf_hip.h")

SIGNATURE = ("int zc_ris_lincomb(zc_ctx *ctx, const uint8_t *in32, const uint64_t *scalars, size_t terms, "
             "const uint64_t *base_scalars, uint8_t *out32, uint8_t *ok, size_t n);")


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
    assert "zc_ris_lincomb" in exported and "zc_ris_lincomb" in z.ALL_SYMBOLS
    assert lib.zc_version().decode().startswith("zerocaf_hip 0.6 ")                  # additive: the ABI number stays


def test_plain_c_caller_gets_bad_arg(lib, tmp_path):
    """A null context, terms = 0, and terms = 8 with a base array (nine scalar slots): ZC_ERR_BAD_ARG, nothing written."""
    import dusk_zerocaf_amd as z
    src = tmp_path / "ris_lincomb.c"
    src.write_text('''
#include "zerocaf_hip.h"
#include <stdio.h>
#include <string.h>
int main(void) {
    uint8_t in[8 * 32] = {0}, out[32], ok[1], clean[32];
    uint64_t k[8 * 5] = {0}, kb[5] = {0};
    zc_ctx *fake = (zc_ctx *)(void *)in;              /* never dereferenced: the limits are checked first */
    int (*lincomb)(zc_ctx *, const uint8_t *, const uint64_t *, size_t, const uint64_t *, uint8_t *, uint8_t *, size_t) = zc_ris_lincomb;
    int a, b, c;
    memset(out, 0xA5, sizeof out);
    memset(clean, 0xA5, sizeof clean);
    ok[0] = 0xA5;
    a = lincomb(0, in, k, 2, kb, out, ok, 1);
    b = lincomb(fake, in, k, 0, kb, out, ok, 1);
    c = lincomb(fake, in, k, ZC_LINCOMB_MAX_TERMS, kb, out, ok, 1);
    printf("%d %d %d\\n", a, b, c);
    return a == ZC_ERR_BAD_ARG && b == ZC_ERR_BAD_ARG && c == ZC_ERR_BAD_ARG && !memcmp(out, clean, 32) && ok[0] == 0xA5 ? 0 : 1;
}
''')
    exe = tmp_path / "ris_lincomb"
    libdir = os.path.dirname(z.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L", libdir, "-lzerocaf_hip", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib"])
    subprocess.check_call([str(exe)])


def test_engine_has_ris_lincomb():
    from dusk_zerocaf_amd.engine import Engine
    assert callable(getattr(Engine, "ris_lincomb", None))


def test_cpp_and_rust_mirrors_call_it():
    hpp = open(os.path.join(ROOT, "dusk_zerocaf_amd", "include", "zerocaf.hpp")).read()
    rs = open(os.path.join(ROOT, "integration", "rust", "zerocaf-hip", "src", "lib.rs")).read()
    ffi = open(os.path.join(ROOT, "integration", "rust", "zerocaf-hip", "src", "ffi.rs")).read()
    assert "zc_ris_lincomb(" in hpp and re.search(r"\bris_lincomb\(const std::vector<std::vector<CompressedRistretto>>&", hpp)
    assert "ffi::zc_ris_lincomb(" in rs and "pub fn ris_lincomb(" in rs
    assert "pub fn zc_ris_lincomb(" in ffi


def test_documents_name_it():
    """README and INTEGRATION.md name the entry point; INTEGRATION.md has its section (4d) with the Schnorr example, DESIGN.md
    the kernel's resource figures."""
    readme = open(os.path.join(ROOT, "README.md")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "zc_ris_lincomb" in readme and "zc_ris_lincomb" in integ and "k_ris_lincomb" in design
    assert re.search(r"^#+ *4d\b", integ, flags=re.M) and "zc_sc_neg" in integ[integ.index("4d."):]
