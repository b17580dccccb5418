#!/usr/bin/env python3
"""SHA-512 over batched rows: the three calls against what a caller did before them, one JSON record.

Device-resident inputs, HIP events on the launch stream.  Per group the paths are warmed up, then timed one after the other in
every one of `--reps` rounds (alternated in this process); a sample is `inner` back-to-back calls between two events, `inner`
chosen per path so that a sample lasts about 20 ms.  Every entry carries a `parity` flag from a comparison of whole outputs in
the same run.  Groups, all at 2^`--lg` rows:
  * challenge:  zc_sc_from_sha512 on rows of 32 + 32 + 32 bytes behind a 6-byte prefix (device-resident R, A, m)  |  the
                composition the documents described before, as a Python caller runs it: download R and A (m is the caller's own,
                on the host already); hashlib.sha512 per row; upload the digests; zc_sc_from_bytes_wide.  The composition is the comparison value, timed with a host clock
                around work that ends in a device synchronise; it is not the code under test.
  * digest:     zc_sha512_rows alone at 1, 2 and 8 blocks per row (one part of 96, 224, 992 bytes, a multiple of 8: the word
                form; and the same rows behind a 6-byte prefix with 6 bytes fewer: the byte form), as blocks/s, as a fraction of
                the integer-VALU issue roof, and as a share of the HBM bandwidth.
  * to_group:   zc_ris_from_sha512  |  zc_ris_from_uniform_bytes on the precomputed digests of the same rows: the difference is
                the cost of the fused hash.
The issue roof: one wave-instruction (64 lanes) per 4 cycles per SIMD x 1024 SIMDs x the shader clock libzc_ubench.so measures
in this run, divided by the VALU instructions per block from the compiler's ISA (`--isa FILE`: the JSON `--count-isa` writes, on
any machine with hipcc; without it the roof is left out).
Usage: python tools/bench_hash.py [--lg 20] [--reps 10] [--warmup 3] [--isa profiles/r17_hash_isa.json] [--out profiles/r17_hash.json]
       python tools/bench_hash.py --count-isa profiles/r17_hash_isa.json          (no GPU needed)"""
import argparse
import collections
import ctypes
import hashlib
import json
import math
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0            # MI355X: 8 TB/s spec
SIMDS = 1024                     # 256 compute units x 4
PREFIX = b"domain"


# ------------------------------------------------------------------ instructions per block, from the compiler's ISA
def count_isa(out_path):
    """VALU instructions of the sixteen-round loop of k_sha512_rows (the innermost loop with the most v_alignbit_b32), counted
    as tools/isa_mix.py counts a loop body.  A block runs five groups of sixteen rounds; the first has no schedule update, so
    5 x the loop overstates the rounds by the schedule's share of one group (about 8 %), and the reader's instructions (16
    loads and byte swaps per block in the word form) are not in it."""
    src = os.path.join(ROOT, "dusk_zerocaf_amd", "csrc", "zerocaf_hip.hip")
    with tempfile.TemporaryDirectory() as d:
        asm = os.path.join(d, "zc.s")
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--offload-device-only", "-o", asm, src], check=True, stderr=subprocess.DEVNULL)
        text = open(asm).read()
    rec = {}
    for kernel in ("k_sha512_rows", "k_sc_from_sha512", "k_ris_from_sha512"):
        i0 = text.index("\n%s:" % kernel)
        body = text[i0:text.index(".Lfunc_end", i0)]
        lines = [l.split(";")[0].strip() for l in body.split("\n")]
        lines = [l for l in lines if l and not l.startswith((".p2align", ".section", ".type", ".globl", "#"))]
        labels = {l[:-1]: i for i, l in enumerate(lines) if re.match(r"^\.LBB\d+_\d+:$", l)}
        loops = []
        for i, l in enumerate(lines):
            m = re.match(r"s_c?branch\w* (\.LBB\d+_\d+)", l)
            if m and labels.get(m.group(1), i) < i:
                loops.append((labels[m.group(1)], i))
        best = None
        for a, b in loops:
            if any(a <= x and y <= b and (x, y) != (a, b) for x, y in loops):
                continue                                                             # not innermost
            ops = collections.Counter(l.split()[0] for l in lines[a:b] if not l.endswith(":"))
            if best is None or ops["v_alignbit_b32"] > best["v_alignbit_b32"]:
                best = ops
        valu = sum(v for k, v in best.items() if k.startswith("v_"))
        rec[kernel] = {"source": "hipcc -S --offload-device-only, the innermost loop with the most v_alignbit_b32 (sixteen rounds)",
                       "valu_per_16_rounds": valu, "valu_per_block_rounds": 5 * valu, "v_alignbit_b32": best["v_alignbit_b32"],
                       "v_mov": sum(v for k, v in best.items() if k.startswith("v_mov")),
                       "scratch_or_buffer_instructions_in_kernel": sum(1 for l in lines if l.startswith(("scratch_", "buffer_"))),
                       "opcodes": {k: v for k, v in best.most_common() if k.startswith("v_")}}
    with open(out_path, "w") as f:
        f.write(json.dumps(rec, indent=1) + "\n")
    print(json.dumps({k: {x: v[x] for x in ("valu_per_16_rounds", "valu_per_block_rounds", "v_alignbit_b32", "v_mov")} for k, v in rec.items()}))
    return 0


# ------------------------------------------------------------------ timing
def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.dtype == np.uint8 else a.view(np.int64)).cuda()


def sample_ms(f, inner, st, host_clock=False):
    import torch
    if host_clock:                                          # work with host stages in it: wall time around a synchronise
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / inner
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(inner):
        f()
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def run_group(paths, reps, warmup, st, host_clock=()):
    import torch
    inner = {}
    for name, f in paths.items():
        for _ in range(1 if name in host_clock else warmup):
            f()
        torch.cuda.synchronize()
        one = sample_ms(f, 1, st, name in host_clock)
        inner[name] = max(1, min(200, math.ceil(20.0 / max(one, 1e-3))))
    times = {name: [] for name in paths}
    for _ in range(reps):
        for name, f in paths.items():
            times[name].append(sample_ms(f, inner[name], st, name in host_clock))
    return {name: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "calls_per_sample": inner[name],
                   "clock": "host clock around a device synchronise" if name in host_clock else "device events"} for name, v in times.items()}


def shader_clock_ghz():
    """The shader clock libzc_ubench.so measures under a saturated integer load in this process (as bench.py reads it)."""
    import dusk_zerocaf_amd as z
    path = os.path.join(os.path.dirname(z.LIB_PATH), "libzc_ubench.so")
    if not os.path.exists(path):
        return None
    ub = ctypes.CDLL(path)
    ub.zc_ubench_mad_u64_u32.restype = ctypes.c_double
    ub.zc_ubench_mad_u64_u32.argtypes = [ctypes.c_double, ctypes.POINTER(ctypes.c_double)]
    ghz = ctypes.c_double(0.0)
    ub.zc_ubench_mad_u64_u32(20.0, ctypes.byref(ghz))
    return ghz.value or None


def hashlib_rows(prefix, arrays):
    n = len(arrays[0])
    return np.frombuffer(b"".join(hashlib.sha512(prefix + b"".join(a[i].tobytes() for a in arrays)).digest() for i in range(n)), dtype=np.uint8).reshape(n, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--isa", default="")
    ap.add_argument("--count-isa", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.count_isa:
        return count_isa(args.count_isa)
    import torch
    import dusk_zerocaf_amd as z
    from tests import scalar_ext_rows as S
    n = 1 << args.lg
    eng = z.Engine([0])
    st = torch.cuda.current_stream()
    eng.set_stream(st.cuda_stream)
    isa = json.load(open(args.isa)) if args.isa else None
    ghz = shader_clock_ghz()
    nominal_ghz = (getattr(torch.cuda.get_device_properties(0), "clock_rate", 0) or 2400000) / 1e6
    rec = {"lib": eng.lib.zc_version().decode(), "device": torch.cuda.get_device_name(0), "rows": n, "reps": args.reps,
           "shader_clock_ghz_in_this_run": ghz and round(ghz, 3), "nominal_clock_ghz": round(nominal_ghz, 3), "isa": isa}
    rng = np.random.default_rng(1700 + args.lg)
    ok = True

    # ---- the Schnorr challenge: device call against the host composition
    R, A, M = (dev(rng.integers(0, 256, size=(n, 32), dtype=np.uint8)) for _ in range(3))
    Mh = M.cpu().numpy()

    def composition():
        rh, ah = R.cpu().numpy(), A.cpu().numpy()
        return eng.sc_from_bytes_wide(dev(hashlib_rows(PREFIX, (rh, ah, Mh))))
    want = composition()
    got = eng.sc_from_sha512([R, A, M], PREFIX)
    parity = bool((got == want).all())
    first = S.canon_rows([int.from_bytes(hashlib.sha512(PREFIX + b"".join(x[0].cpu().numpy().tobytes() for x in (R, A, M))).digest(), "little")])[0]
    parity = parity and bool((got[0].cpu().numpy().view(np.uint64) == first).all())
    print("challenge parity", parity, file=sys.stderr, flush=True)
    ok = ok and parity
    ch = run_group({"zc_sc_from_sha512": lambda: eng.sc_from_sha512([R, A, M], PREFIX), "download_hashlib_upload_sc_from_bytes_wide": composition},
                   args.reps, args.warmup, st, host_clock=("download_hashlib_upload_sc_from_bytes_wide",))
    ch["parity"] = parity
    ch["composition_over_device_call"] = round(ch["download_hashlib_upload_sc_from_bytes_wide"]["median_ms"] / ch["zc_sc_from_sha512"]["median_ms"], 1)
    ch["device_call_below_composition"] = ch["zc_sc_from_sha512"]["median_ms"] < ch["download_hashlib_upload_sc_from_bytes_wide"]["median_ms"]
    rec["challenge"] = ch

    # ---- the digest alone
    rec["digest"] = []
    for blocks, nbytes in ((1, 96), (2, 224), (8, 992)):
        for form, prefix, length in (("word", b"", nbytes), ("byte", PREFIX, nbytes - len(PREFIX))):
            assert (len(prefix) + length + 17 + 127) // 128 == blocks
            part = dev(rng.integers(0, 256, size=(n, length), dtype=np.uint8))
            out = eng.sha512_rows([part], prefix)
            idx = np.unique(np.concatenate([np.arange(0, n, max(1, n // 4096)), [n - 1]]))
            parity = bool((out.cpu().numpy()[idx] == hashlib_rows(prefix, (part.cpu().numpy()[idx],))).all())
            print("digest %d blocks, %s form: parity %s" % (blocks, form, parity), file=sys.stderr, flush=True)
            ok = ok and parity
            r = run_group({"zc_sha512_rows": lambda: eng.sha512_rows([part], prefix)}, args.reps, args.warmup, st)["zc_sha512_rows"]
            ms = r["median_ms"]
            bytes_per_row = length + 64
            r.update({"blocks_per_row": blocks, "reader_form": form, "prefix_len": len(prefix), "part_len": length, "parity": parity,
                      "parity_rows_checked": int(len(idx)), "G_blocks_per_s": round(blocks * n / ms / 1e6, 3), "M_rows_per_s": round(n / ms / 1e3, 1),
                      "bytes_per_row": bytes_per_row, "alg_GBps": round(bytes_per_row * n / ms / 1e6, 1),
                      "hbm_share": round(bytes_per_row * n / ms / 1e6 / HBM_PEAK_GBS, 4)})
            if isa and ghz:
                valu = isa["k_sha512_rows"]["valu_per_block_rounds"]
                roof = SIMDS * ghz * 1e9 / 4 * 64 / valu                             # blocks/s with every SIMD issuing one VALU instruction per 4 cycles
                r.update({"issue_roof_G_blocks_per_s": round(roof / 1e9, 3), "fraction_of_issue_roof": round(blocks * n / ms * 1e3 / roof, 4)})
                r["bound"] = "integer VALU issue" if r["fraction_of_issue_roof"] > r["hbm_share"] else "HBM"
            rec["digest"].append(r)
            del part, out
            torch.cuda.empty_cache()

    # ---- hash-to-group against the same rows' precomputed digests
    dig = eng.sha512_rows([R, A, M], PREFIX)
    parity = bool((eng.ris_from_sha512([R, A, M], PREFIX) == eng.ris_from_uniform_bytes(dig)).all())
    print("to_group parity", parity, file=sys.stderr, flush=True)
    ok = ok and parity
    tg = run_group({"zc_ris_from_sha512": lambda: eng.ris_from_sha512([R, A, M], PREFIX), "zc_ris_from_uniform_bytes": lambda: eng.ris_from_uniform_bytes(dig)},
                   args.reps, args.warmup, st)
    tg["parity"] = parity
    tg["cost_of_the_fused_hash_ms"] = round(tg["zc_ris_from_sha512"]["median_ms"] - tg["zc_ris_from_uniform_bytes"]["median_ms"], 4)
    rec["to_group"] = tg
    eng.close()
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
