"""CPU tier: the fixed-base MSM entry points (ABI 0.6) are declared, exported, callable from plain C and mirrored in Python.
(No GPU: every call here fails on its arguments before a device is touched.)"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zerocaf_hip.h")

SIGNATURES = {
    "zc_msm_bases_create": "int zc_msm_bases_create(zc_ctx *ctx, const uint64_t *points, size_t n, int window_bits, uint64_t *id_out);",
    "zc_msm_bases_destroy": "int zc_msm_bases_destroy(zc_ctx *ctx, uint64_t id);",
    "zc_msm_fixed": "int zc_msm_fixed(zc_ctx *ctx, uint64_t id, const uint64_t *scalars, size_t batch, uint64_t *out_points);",
    "zc_msm_fixed_plan": "int zc_msm_fixed_plan(zc_ctx *ctx, size_t n, int window_bits, int32_t *out, int nout);",
}


@pytest.fixture(scope="module")
def lib():
    import dusk_zerocaf_amd as z
    if not os.path.exists(z.LIB_PATH):
        from dusk_zerocaf_amd import build
        build.build(test_hooks=True)
    return z.load()


def test_header_declares_the_fixed_base_entry_points():
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
    src = tmp_path / "fixed.c"
    src.write_text('''
#include "zerocaf_hip.h"
#include <stdio.h>
int main(void) {
    uint64_t pts[20] = {0}, k[5] = {0}, out[20], id = 0;
    int32_t plan[8];
    int (*create)(zc_ctx *, const uint64_t *, size_t, int, uint64_t *) = zc_msm_bases_create;
    int (*destroy)(zc_ctx *, uint64_t) = zc_msm_bases_destroy;
    int (*fixed)(zc_ctx *, uint64_t, const uint64_t *, size_t, uint64_t *) = zc_msm_fixed;
    int (*query)(zc_ctx *, size_t, int, int32_t *, int) = zc_msm_fixed_plan;
    int a = create(0, pts, 1, 0, &id), b = destroy(0, 1), c = fixed(0, 1, k, 1, out), d = query(0, 1, 0, plan, 8);
    printf("%d %d %d %d %llu\\n", a, b, c, d, (unsigned long long)id);
    return a == ZC_ERR_BAD_ARG && b == ZC_ERR_BAD_ARG && c == ZC_ERR_BAD_ARG && d == ZC_ERR_BAD_ARG && id == 0 ? 0 : 1;
}
''')
    exe = tmp_path / "fixed"
    libdir = os.path.dirname(z.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L", libdir, "-lzerocaf_hip", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib"])
    subprocess.check_call([str(exe)])


def test_engine_has_msm_bases():
    from dusk_zerocaf_amd.engine import Engine, MsmBases
    assert callable(getattr(Engine, "msm_bases", None)) and callable(getattr(Engine, "msm_fixed_plan", None))
    for m in ("msm", "close", "__enter__", "__exit__"):
        assert callable(getattr(MsmBases, m, None)), m
