"""CPU tier: the C-ABI library loads and exports every symbol include/zerocaf_hip.h declares
(no compute without a GPU), and refuses to work without a device instead of falling back."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zerocaf_hip.h")


def declared_symbols():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(zc_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    import dusk_zerocaf_amd as z
    if not os.path.exists(z.LIB_PATH):
        from dusk_zerocaf_amd import build
        build.build(test_hooks=True)
    return z.load()


def test_header_declares_the_path():
    syms = declared_symbols()
    for must in ("zc_fe_mul", "zc_fe_square", "zc_fe_invert", "zc_sc_mul", "zc_ed_add", "zc_ed_double",
                 "zc_ed_scalar_mul", "zc_ed_mul_by_pow_2", "zc_ed_compress", "zc_ed_decompress",
                 "zc_ris_compress", "zc_ris_decompress", "zc_ris_roundtrip_mul", "zc_msm"):
        assert must in syms


def test_library_exports_every_declared_symbol(lib):
    import dusk_zerocaf_amd as z
    syms = declared_symbols()
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, missing
    assert sorted(z.ALL_SYMBOLS) == syms                 # the ctypes table mirrors the header exactly
    out = subprocess.check_output(["nm", "-D", "--defined-only", z.LIB_PATH], text=True)
    exported = set(re.findall(r"\bT (zc_[a-z0-9_]+)", out))
    assert set(syms) <= exported
    assert "sum_rows_launch" not in out and "dlog_launches_on" not in out and "_GLOBAL__N_" not in out      # the host helpers stay internal


def test_no_cpu_fallback_and_no_oracle_linkage(lib):
    import dusk_zerocaf_amd as z
    out = subprocess.check_output(["nm", "-D", z.LIB_PATH], text=True)
    assert "zr_" not in out                              # nothing from oracle/ is linked in
    if lib.zc_device_count() == 0:
        with pytest.raises(z.ZerocafHipError):
            z.Engine()                                   # fails loudly: status ZC_ERR_NO_DEVICE
    for root, _, files in os.walk(os.path.join(ROOT, "dusk_zerocaf_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".hpp", ".cpp")):
                src = open(os.path.join(root, f)).read()
                assert "zc_ref" not in src and "from oracle" not in src and "import oracle" not in src, f


def test_release_library_carries_no_test_hooks_and_reads_its_knobs_once(lib):
    """Fault injection (ZC_TEST_RING_POISON / ZC_TEST_RING_SPINS) and the stage hooks (zc_test_*) exist only in
    libzerocaf_hip_test.so, the -DZC_TEST_HOOKS build the GPU test tier loads beside the product; the release library
    has neither the symbols nor the strings.  Tuning knobs are read in ONE place (tuning_from_env, at zc_ctx_create)."""
    import dusk_zerocaf_amd as z
    from dusk_zerocaf_amd import _lib
    rel = subprocess.check_output(["nm", "-D", "--defined-only", z.LIB_PATH], text=True)
    assert "zc_test_" not in rel
    assert b"ZC_TEST_" not in open(z.LIB_PATH, "rb").read()
    tst = subprocess.check_output(["nm", "-D", "--defined-only", _lib.TEST_LIB_PATH], text=True)
    assert {"zc_test_msm_sort", "zc_test_odd_table", "zc_test_staged_launches", "zc_test_launch_forms"} <= set(re.findall(r"\bT (zc_[a-z0-9_]+)", tst))
    assert set(re.findall(r"\bT (zc_[a-z0-9_]+)", rel)) == set(re.findall(r"\bT (zc_[a-z0-9_]+)", tst)) - {"zc_test_msm_sort", "zc_test_odd_table", "zc_test_staged_launches", "zc_test_launch_forms"}
    src = ""
    for f in os.listdir(os.path.join(ROOT, "dusk_zerocaf_amd", "csrc")):
        if f.endswith((".hip", ".h")):
            src += open(os.path.join(ROOT, "dusk_zerocaf_amd", "csrc", f)).read()
    body = src[src.index("Tuning tuning_from_env()"):]
    body = body[:body.index("\n}\n")]
    outside = src.replace(body, "")
    assert re.findall(r"getenv\(\"(ZC_[A-Z_0-9]+)\"\)", outside) == ["ZC_RCCL_PATH"]     # where librccl lives: not a tuning knob
    # the product's knob surface, from the shipped binary itself: nine tuning knobs.  The path
    # forcers of the test tier exist in the -DZC_TEST_HOOKS build only; variants that were measured and lost are compile-time
    # macros (build_variant), not switches
    strings = lambda path: set(re.findall(rb"\x00(ZC_[A-Z][A-Z_0-9]+)(?=\x00)", open(path, "rb").read()))     # whole C strings
    product = sorted(x.decode() for x in strings(z.LIB_PATH) if not x.startswith((b"ZC_ERR", b"ZC_OK")))
    assert product == ["ZC_HOST_CHUNKS", "ZC_INV_CHUNK", "ZC_JACOBI_ROUNDS", "ZC_MSM_AFFINE", "ZC_MSM_GROUPS", "ZC_MSM_WINDOW", "ZC_RCCL_PATH",
                       "ZC_RING_SLOTS", "ZC_RISTRETTO_STRICT", "ZC_SCHED"], product
    hooks_only = sorted(x.decode() for x in strings(_lib.TEST_LIB_PATH) - strings(z.LIB_PATH))
    assert hooks_only == ["ZC_MSM_AFFINE_CHUNK", "ZC_MSM_FORK", "ZC_MSM_RUN", "ZC_MSM_RUN_EDGES", "ZC_MSM_SEG", "ZC_MSM_SORT_BIG", "ZC_MSM_SORT_G",
                          "ZC_MSM_SORT_PACKED", "ZC_TEST_LAUNCH_FAIL", "ZC_TEST_RING_POISON", "ZC_TEST_RING_SPINS", "ZC_TEST_STREAM_MIN_BYTES"], hooks_only
    assert "PROBE" not in src                                # timing probes live in tools/debug/probes/*.patch
    assert "env_long(" in body and outside.count("env_long(") == 1                      # its definition only


def test_documents_quote_the_real_entry_point_count():
    """INTEGRATION.md and README.md name the number of entry points; it must be the header's."""
    n = len(declared_symbols())
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "**all %d** entry points" % n in integ and "\n%d entry points (" % n in integ
    assert "%d entry points" % n in open(os.path.join(ROOT, "README.md")).read()


def test_rust_shim_binds_the_whole_abi():
    """integration/rust/zerocaf-hip (source only: no Rust toolchain here) declares every entry
    point of the header -- ffi.rs is generated from it -- and its safe layer calls each one."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_rust_ffi", os.path.join(ROOT, "tools", "gen_rust_ffi.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    ffi = open(gen.OUT).read()
    assert ffi == gen.render(), "run tools/gen_rust_ffi.py"
    declared = set(re.findall(r"pub fn (zc_[a-z0-9_]+)\(", ffi))
    assert declared == set(declared_symbols())
    shim = open(os.path.join(os.path.dirname(gen.OUT), "lib.rs")).read()
    used = set(re.findall(r"ffi::(zc_[a-z0-9_]+)", shim))
    assert used == declared, sorted(declared - used)


def test_cpp_mirror_covers_the_whole_abi():
    """dusk_zerocaf_amd/include/zerocaf.hpp (the C++ host-side mirror) reaches every entry point."""
    hpp = open(os.path.join(ROOT, "dusk_zerocaf_amd", "include", "zerocaf.hpp")).read()
    missing = [s for s in declared_symbols() if s + "(" not in hpp]
    assert not missing, missing


def test_header_is_plain_c_and_links(lib, tmp_path):
    """The boundary a Rust `extern "C"` block (or cgo, JNI ...) binds must be C-clean: compile
    include/zerocaf_hip.h as C11 with warnings as errors and call the GPU-free entry points from C."""
    import dusk_zerocaf_amd as z
    src = tmp_path / "abi.c"
    src.write_text('''
#include "zerocaf_hip.h"
#include <stdio.h>
int main(void) {
    zc_ctx *ctx = 0;
    int (*fn)(zc_ctx *, const uint64_t *, const uint64_t *, uint64_t *, size_t, unsigned) = zc_ed_scalar_mul;
    printf("%s|%d|%d\\n", zc_version(), zc_device_count() >= 0, fn != 0);
    if (zc_device_count() == 0) return zc_ctx_create(0, 0, &ctx) == ZC_ERR_NO_DEVICE ? 0 : 3;
    return 0;
}
''')
    exe = tmp_path / "abi"
    libdir = os.path.dirname(z.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L", libdir, "-lzerocaf_hip", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.check_output([str(exe)], text=True)
    assert out.startswith("zerocaf_hip") and out.strip().endswith("|1|1")


def test_engine_binds_torch_streams_to_the_slot_that_owns_the_tensor():
    """A multi-device Engine keeps one stream per context slot: following torch's current stream must bind it to the
    slot of the TENSOR's device (zc_ctx_set_stream_dev), and a tensor on a device outside the context is refused
    before anything is launched.  (No GPU needed: the library call is recorded, not made.)"""
    import types
    import dusk_zerocaf_amd as z
    from dusk_zerocaf_amd.engine import Engine
    calls = []
    e = Engine.__new__(Engine)
    e.ctx, e._pinned_stream, e._last_torch_stream, e._devices = None, False, {}, [2, 5]
    e.lib = types.SimpleNamespace(zc_ctx_set_stream_dev=lambda ctx, slot, h, ext: calls.append((slot, h.value, ext)) or 0)
    import torch
    handle = {2: 0x1000, 5: 0x2000}
    orig = torch.cuda.current_stream
    torch.cuda.current_stream = lambda dev=None: types.SimpleNamespace(cuda_stream=handle[dev.index])
    try:
        t2 = types.SimpleNamespace(device=types.SimpleNamespace(index=2))
        t5 = types.SimpleNamespace(device=types.SimpleNamespace(index=5))
        e._follow_torch_stream(t5)
        e._follow_torch_stream(t2)
        e._follow_torch_stream(t5)                           # cached per slot: no second call
        assert calls == [(1, 0x2000, 1), (0, 0x1000, 1)]
        with pytest.raises(z.ZerocafHipError):
            e._follow_torch_stream(types.SimpleNamespace(device=types.SimpleNamespace(index=3)))
    finally:
        torch.cuda.current_stream = orig
        e.ctx = None


def test_default_engine_knows_its_device_so_the_ownership_check_always_runs():
    """`Engine()` (no device list) used to keep `_devices = None`, and a tensor on another GPU then got that
    GPU's torch stream bound to slot 0.  The constructor now always records the context's devices -- torch's current device
    when torch sees a GPU; otherwise zc_ctx_create(NULL, 0), i.e. whatever device the caller's hipSetDevice
    chose, read back through zc_ctx_device -- so a foreign tensor is refused before anything is launched.  (No GPU needed:
    a stand-in for the library records the zc_ctx_create call.)"""
    import types
    import dusk_zerocaf_amd as z
    from dusk_zerocaf_amd.engine import Engine
    seen = []

    def create(arr, n, out):
        seen.append(None if arr is None else [arr[i] for i in range(n)])
        return 0
    fake = types.SimpleNamespace(zc_ctx_create=create, zc_ctx_destroy=lambda ctx: 0, zc_last_error=lambda: b"",
                                 zc_ctx_set_stream_dev=lambda ctx, slot, h, ext: 0,
                                 zc_ctx_device=lambda ctx, slot: 3, zc_ctx_device_count=lambda ctx: 1)
    e = Engine(lib=fake)
    assert seen == [None] and e._devices == [3]                 # no torch GPU here: the library's own choice (the current HIP device), read back
    e.ctx = None
    fake.zc_ctx_device = lambda ctx, slot: 0
    e = Engine(lib=fake)
    import torch
    orig = torch.cuda.current_stream
    torch.cuda.current_stream = lambda dev=None: types.SimpleNamespace(cuda_stream=0x1234)
    try:
        with pytest.raises(z.ZerocafHipError, match="owns devices"):
            e._follow_torch_stream(types.SimpleNamespace(device=types.SimpleNamespace(index=1)))
        e._follow_torch_stream(types.SimpleNamespace(device=types.SimpleNamespace(index=0)))
    finally:
        torch.cuda.current_stream = orig
        e.ctx = None
