"""GPU tier: the C++ host-side mirror (dusk_zerocaf_amd/include/zerocaf.hpp) reproduces the
reference's own unit-test assertions through the C ABI (tests/cpp/test_zerocaf_hpp.cpp)."""
import os
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_mirror_reference_style_checks():
    src = os.path.join(ROOT, "tests", "cpp", "test_zerocaf_hpp.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "test_zerocaf_hpp")
    libdir = os.path.join(ROOT, "dusk_zerocaf_amd")
    hpp = os.path.join(ROOT, "dusk_zerocaf_amd", "include", "zerocaf.hpp")
    newest = max(os.path.getmtime(src), os.path.getmtime(hpp))
    if shutil.which("g++") and (not os.path.exists(exe) or os.path.getmtime(exe) < newest):
        subprocess.check_call(["g++", "-O1", "-std=c++17", src, "-o", exe, "-L", libdir, "-lzerocaf_hip",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"])
    env = dict(os.environ, LD_LIBRARY_PATH=libdir + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all reference-style checks passed" in out.stdout


def test_cpp_mirror_extended_wrappers(tmp_path):
    """Every wrapper the program above does not run (tests/cpp/test_zerocaf_hpp_ext.cpp), against the composed operators; the
    plans it prints are the ones the Python Engine reports for the same sizes.  Built into tmp_path, run once."""
    import time
    if not shutil.which("g++"):
        pytest.skip("no g++")
    src = os.path.join(ROOT, "tests", "cpp", "test_zerocaf_hpp_ext.cpp")
    exe = str(tmp_path / "test_zerocaf_hpp_ext")
    libdir = os.path.join(ROOT, "dusk_zerocaf_amd")
    rocm_root = os.environ.get("ROCM_PATH", "/opt/rocm")
    rocm = os.path.join(rocm_root, "lib")
    # (hip_runtime_api.h is plain C++ for g++ once the platform is named: the prototypes and hipMemcpyDeviceToHost come from ROCm)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-D__HIP_PLATFORM_AMD__", "-isystem", os.path.join(rocm_root, "include"), src, "-o", exe,
                           "-L", libdir, "-lzerocaf_hip", "-L", rocm, "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath," + rocm, "-Wl,-rpath-link," + rocm])
    env = dict(os.environ, LD_LIBRARY_PATH=libdir + ":" + rocm + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    t0 = time.perf_counter()
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    print("test_zerocaf_hpp_ext: %.1f s" % (time.perf_counter() - t0))
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all extended checks passed" in out.stdout and "FAIL" not in out.stdout
    import re
    ran = {tok for l in out.stdout.splitlines() if l.startswith("ran ") for tok in re.findall(r"[A-Za-z_][A-Za-z0-9_]*", l)}      # whole names
    for wrapper in ("fold_ordered", "msm_partial", "double_and_compress_batch", "window_naf_mul_batch", "msm_batch", "ed_lincomb", "ris_lincomb", "ris_lincomb_sum",
                    "scalar_mul_shared", "ris_mul_shared", "ed_lincomb_shared", "ris_lincomb_shared", "sha512_rows", "sc_from_sha512", "ris_from_sha512", "MsmBases",
                    "Generators", "sum_rows", "from_bytes_wide", "from_bytes_mod_order", "muladd", "invert", "set_stream", "host_register"):
        assert wrapper in ran, wrapper
    import dusk_zerocaf_amd as z
    e = z.Engine()
    try:
        plans = [l.split() for l in out.stdout.splitlines() if l.startswith("plan ")]
        assert len(plans) == 6
        for _, kind, a, b, *v in plans:
            v = [int(x) for x in v]
            assert len(v) == 8
            if kind == "msm_batch":
                p = e.msm_batch_plan(int(a), int(b))
                want = [1 if p["regime"] == "buckets" else 0, p["window_bits"], p["windows"], int(p["affine"]), p["run"], p["segment_buckets"], p["sort_passes"], p["record_stride"]]
            else:
                p = e.msm_fixed_plan(int(a), int(b))
                want = [p["window_bits"], p["windows"], p["record_stride"], p["run"], p["segment_buckets"], p["sort_passes"], p["table_mib"], p["window_groups"]]
            assert v == want, (kind, a, b, v, want)
    finally:
        e.close()
