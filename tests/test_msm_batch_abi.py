"""CPU tier: the batched variable-base MSM entry points (zc_msm_batch, zc_msm_batch_plan) are declared, exported, callable
from plain C and mirrored in Python, C++ and Rust.  (No GPU: every call here fails on its arguments before a device is touched.)"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zerocaf_hip.h")

SIGNATURES = {
    "zc_msm_batch": "int zc_msm_batch(zc_ctx *ctx, const uint64_t *points, const uint64_t *scalars, size_t n, size_t batch, "
                    "uint64_t *out_points);",
    "zc_msm_batch_plan": "int zc_msm_batch_plan(zc_ctx *ctx, size_t n, size_t batch, int points_aligned16, int32_t *out, int nout);",
}


@pytest.fixture(scope="module")
def lib():
    import dusk_zerocaf_amd as z
    if not os.path.exists(z.LIB_PATH):
        from dusk_zerocaf_amd import build
        build.build(test_hooks=True)
    return z.load()


def test_header_declares_the_batch_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decls = " ".join(text.split())
    for name, sig in SIGNATURES.items():
        assert " ".join(sig.split()) in decls, name


def test_library_exports_them(lib):
    import dusk_zerocaf_amd as z
    out = subprocess.check_output(["nm", "-D", "--defined-only", z.LIB_PATH], text=True)
    exported = set(re.findall(r"\bT (zc_[a-z0-9_]+)", out))
    assert set(SIGNATURES) <= exported
    assert set(SIGNATURES) <= set(z.ALL_SYMBOLS)
    assert lib.zc_version().decode().startswith("zerocaf_hip 0.6 ")


def test_plain_c_caller_gets_bad_arg_without_a_context(lib, tmp_path):
    import dusk_zerocaf_amd as z
    src = tmp_path / "batch.c"
    src.write_text('''
#include "zerocaf_hip.h"
#include <stdio.h>
int main(void) {
    uint64_t pts[40] = {0}, k[10] = {0}, out[40];
    int32_t plan[8];
    int (*batch)(zc_ctx *, const uint64_t *, const uint64_t *, size_t, size_t, uint64_t *) = zc_msm_batch;
    int (*query)(zc_ctx *, size_t, size_t, int, int32_t *, int) = zc_msm_batch_plan;
    int a = batch(0, pts, k, 1, 2, out), b = query(0, 1, 2, 1, plan, 8);
    printf("%d %d\\n", a, b);
    return a == ZC_ERR_BAD_ARG && b == ZC_ERR_BAD_ARG ? 0 : 1;
}
''')
    exe = tmp_path / "batch"
    libdir = os.path.dirname(z.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L", libdir, "-lzerocaf_hip", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib"])
    subprocess.check_call([str(exe)])


def test_engine_has_msm_batch():
    from dusk_zerocaf_amd.engine import Engine
    assert callable(getattr(Engine, "msm_batch", None)) and callable(getattr(Engine, "msm_batch_plan", None))


def test_cpp_and_rust_mirrors_call_it():
    hpp = open(os.path.join(ROOT, "dusk_zerocaf_amd", "include", "zerocaf.hpp")).read()
    rs = open(os.path.join(ROOT, "integration", "rust", "zerocaf-hip", "src", "lib.rs")).read()
    assert "zc_msm_batch(" in hpp and re.search(r"inline std::vector<EdwardsPoint> msm_batch\(", hpp)
    assert "ffi::zc_msm_batch(" in rs and "pub fn msm_batch(" in rs
    assert "zc_msm_batch_plan(" in hpp and "ffi::zc_msm_batch_plan(" in rs
