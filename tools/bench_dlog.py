#!/usr/bin/env python3
"""Bounded discrete logs (zc_dlog_create, zc_ed_dlog, zc_ris_dlog), device-resident, the figures of one shape alternated in one
process.  Writes profiles/r22_dlog.json.

Per shape: WARMUP untimed rounds, then REPEATS rounds in which every path runs once, one after the other; a sample is the wall
time between two device synchronisations of one call.  Reported per path: median, minimum, maximum and spread =
(max - min) / median of the samples.  Every row's m is PLANTED: P = m * B from zc_ed_mul_base (the wire rows its zc_ris_compress),
and every shape is checked first: found everywhere, m as planted ("parity").

  random   m uniform below the bound
  worst    every row in the last giant step: m = bound - 1 - (i mod 2^t), so a wave walks all ceil(bound / 2^t) steps

--ab-lib PATH --ab-chunk C: the first shape once more on the product and on a build with another DLOG_CHUNK (python -m
dusk_zerocaf_amd.build --variant NAME ZC_DLOG_CHUNK=C), two contexts on the device, alternated: the key chunk_ab.

Create time: zc_dlog_create + zc_dlog_destroy at 2^16 / 2^20 / 2^22 records, plain and COSET4 alternated.

The baseline is the composition a caller can write without these calls, at 2^16 records, bound 2^20, 2^16 rows: per giant step
zc_ed_add with the stride tiled, zc_ed_to_affine, a download, a sorted-key lookup in numpy; the call is measured at the same
shape.

Multiplications per giant step are COUNTED, not measured: 7 (mixed addition) + 2 (U = Y a, a = a Z) + 2 (y = U I, I = I Z) = 11,
plus one division-step inversion per DLOG_CHUNK steps.  roof_fraction prices those 11 at 135 v_mad_u64_u32 each against the
measured 32.0 T lane-ops/s of that instruction (profiles/roofline_inputs.json)."""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import pymodel as pm  # noqa: E402
WARMUP, REPEATS = 2, 7
MULS_PER_STEP, MADS_PER_MUL, MAD_LANE_OPS_PER_S = 11, 135, 32.0e12


def limbs(m):
    m = np.asarray(m, dtype=np.uint64)
    out = np.zeros((len(m), 5), dtype=np.uint64)
    out[:, 0] = m & np.uint64((1 << 52) - 1)
    out[:, 1] = m >> np.uint64(52)
    return out


def main():
    import torch
    import dusk_zerocaf_amd as z
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_dlog.json"))
    ap.add_argument("--quick", action="store_true", help="the first shape and the baseline only")
    ap.add_argument("--chunk", type=int, default=0, help="DLOG_CHUNK of the library under test when it is an A/B build (ZC_LIB_PATH)")
    ap.add_argument("--ab-lib", default=None, help="a second build of the library (python -m dusk_zerocaf_amd.build --variant NAME ZC_DLOG_CHUNK=c): "
                    "the first shape is measured on both, alternated, into the key chunk_ab")
    ap.add_argument("--ab-chunk", type=int, default=0, help="its DLOG_CHUNK")
    args = ap.parse_args()
    eng = z.Engine()
    rng = np.random.default_rng(22)
    i64 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()
    chunk = args.chunk or int(re.search(r"^#define ZC_DLOG_CHUNK (\d+)$", open(os.path.join(ROOT, "dusk_zerocaf_amd", "csrc", "zc_dlog_plan.h")).read(), flags=re.M).group(1))
    B = np.array([sum(pm.pt_limbs(pm.BASEPOINT), [])], dtype=np.uint64)

    def sync():
        torch.cuda.synchronize()
        eng.synchronize()

    def stats(s):
        med = float(np.median(s))
        return {"median_ms": med, "min_ms": min(s), "max_ms": max(s), "spread": (max(s) - min(s)) / med, "samples_ms": s}

    def measure(paths):
        for _ in range(WARMUP):
            for fn in paths.values():
                fn()
        sync()
        samples = {name: [] for name in paths}
        for _ in range(REPEATS):
            for name, fn in paths.items():
                sync()
                t0 = time.perf_counter()
                fn()
                sync()
                samples[name].append((time.perf_counter() - t0) * 1e3)
        return {name: stats(s) for name, s in samples.items()}

    def planted(n, t, bound, kind):
        if kind == "random":
            m = rng.integers(0, bound, size=n, dtype=np.uint64)
        else:
            m = np.uint64(bound - 1) - (np.arange(n, dtype=np.uint64) & np.uint64((1 << t) - 1))
        pts = eng.ed_mul_base(i64(limbs(m)))
        return m, pts, eng.ris_compress(pts)

    def check(res, m):
        got, found, ok = (x.cpu().numpy() for x in res)
        return bool(found.all() and ok.all() and np.array_equal(got.view(np.uint64), m))

    results = {"tool": "tools/bench_dlog.py", "device": torch.cuda.get_device_name(0), "warmup": WARMUP, "repeats": REPEATS, "dlog_chunk": chunk,
               "multiplications_per_step_by_count": MULS_PER_STEP, "inversions_per_step": 1.0 / chunk, "create": [], "shapes": []}
    # ---- create
    for t in (16, 20, 22):
        def create(coset4):
            tb = eng.dlog_table(B, t, coset4=coset4)
            tb.close()
        r = measure({"plain": lambda: create(False), "coset4": lambda: create(True)})
        results["create"].append({"table_bits": t, "table_MB_per_device": 48 * (1 << t) / 1e6, "paths": r})
        print("create t=%d: %.1f ms plain, %.1f ms coset4" % (t, r["plain"]["median_ms"], r["coset4"]["median_ms"]), flush=True)
        if args.quick:
            break
    # ---- the calls
    parity_all = True
    for t, lg_bound, lg_n in ((16, 24, 20), (20, 32, 16), (22, 32, 18)):
        bound, n = 1 << lg_bound, 1 << lg_n
        plain, coset = eng.dlog_table(B, t), eng.dlog_table(B, t, coset4=True)
        rows = {kind: planted(n, t, bound, kind) for kind in ("random", "worst")}
        paths, parity = {}, {}
        for kind, (m, pts, enc) in rows.items():
            paths["ed_" + kind] = lambda pts=pts: plain.ed(pts, bound)
            paths["ris_" + kind] = lambda enc=enc: coset.ris(enc, bound)
            parity["ed_" + kind] = check(plain.ed(pts, bound), m)
            parity["ris_" + kind] = check(coset.ris(enc, bound), m)
        r = measure(paths)
        steps = bound >> t
        for name in r:
            r[name]["M_row_steps_per_s_at_all_steps"] = n * steps / r[name]["median_ms"] / 1e3
        worst = r["ed_worst"]
        worst["roof_fraction"] = n * steps / (worst["median_ms"] * 1e-3) * MULS_PER_STEP * MADS_PER_MUL / MAD_LANE_OPS_PER_S
        parity_all = parity_all and all(parity.values())
        results["shapes"].append({"table_bits": t, "bound_log2": lg_bound, "n": n, "giant_steps": steps, "launches": -(-steps // 1024), "parity": parity, "paths": r})
        print("t=%d bound 2^%d n 2^%d: ed %.1f / %.1f ms, ris %.1f / %.1f ms (random / worst), parity %s" % (
            t, lg_bound, lg_n, r["ed_random"]["median_ms"], r["ed_worst"]["median_ms"], r["ris_random"]["median_ms"], r["ris_worst"]["median_ms"], all(parity.values())), flush=True)
        plain.close()
        coset.close()
        del rows, paths
        if args.quick:
            break
    # ---- DLOG_CHUNK A/B: the product and a variant build in one process, two contexts on the device, first shape, alternated
    if args.ab_lib:
        from dusk_zerocaf_amd import _lib
        other = z.Engine(lib=_lib._bind(args.ab_lib))
        t, bound, n = 16, 1 << 24, 1 << 20
        tabs = {"chunk%d" % chunk: (eng.dlog_table(B, t), eng.dlog_table(B, t, coset4=True)), "chunk%d" % args.ab_chunk: (other.dlog_table(B, t), other.dlog_table(B, t, coset4=True))}
        rows = {kind: planted(n, t, bound, kind) for kind in ("random", "worst")}
        paths, parity = {}, True
        for label, (plain, coset) in tabs.items():
            for kind, (m, pts, enc) in rows.items():
                paths["%s_ed_%s" % (label, kind)] = lambda plain=plain, pts=pts: plain.ed(pts, bound)
                parity = parity and check(plain.ed(pts, bound), m)
            m, pts, enc = rows["worst"]
            paths["%s_ris_worst" % label] = lambda coset=coset, enc=enc: coset.ris(enc, bound)
            parity = parity and check(coset.ris(enc, bound), m)
        r = measure(paths)
        results["chunk_ab"] = {"table_bits": t, "bound_log2": 24, "n": n, "product_chunk": chunk, "variant_chunk": args.ab_chunk, "variant": os.path.basename(args.ab_lib), "parity": parity, "paths": r}
        parity_all = parity_all and parity
        print("chunk A/B: " + ", ".join("%s %.1f ms" % (k, v["median_ms"]) for k, v in r.items()), flush=True)
        for pair in tabs.values():
            for tb in pair:
                tb.close()
        other.close()
        del rows, paths
    # ---- the composition without the calls: t = 16, bound 2^20, 2^16 rows
    t, bound, n = 16, 1 << 20, 1 << 16
    T = 1 << t
    m, pts, _ = planted(n, t, bound, "random")
    key64 = lambda xy: xy[:, 5] | (xy[:, 6] << np.uint64(52))                          # the low 64 bits of y: the sort key; all ten limbs decide
    table = np.ascontiguousarray(eng.ed_to_affine(eng.ed_mul_base(i64(limbs(np.arange(T, dtype=np.uint64)))))[0].cpu().numpy().view(np.uint64))
    order = np.argsort(key64(table), kind="stable")
    sorted_keys = key64(table)[order]
    stride = eng.ed_neg(eng.ed_mul_base(i64(limbs(np.array([T], dtype=np.uint64))))).repeat(n, 1).contiguous()

    def composed():
        out, found = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=bool)
        Q = pts
        for g in range(bound >> t):
            a = np.ascontiguousarray(eng.ed_to_affine(Q)[0].cpu().numpy().view(np.uint64))
            at = order[np.minimum(np.searchsorted(sorted_keys, key64(a)), T - 1)]
            hit = (table[at] == a).all(axis=1) & ~found
            out[hit] = np.uint64(g * T) + at[hit].astype(np.uint64)
            found |= hit
            Q = eng.ed_add(Q, stride)
        return out, found
    with eng.dlog_table(B, t) as tb:
        cm, cf = composed()
        parity = bool(cf.all() and np.array_equal(cm, m)) and check(tb.ed(pts, bound), m)
        r = measure({"ed_dlog": lambda: tb.ed(pts, bound), "add_to_affine_download_numpy_lookup": composed})
    r["ed_dlog"]["over_composition"] = r["ed_dlog"]["median_ms"] / r["add_to_affine_download_numpy_lookup"]["median_ms"]
    parity_all = parity_all and parity
    results["composition"] = {"table_bits": t, "bound_log2": 20, "n": n, "giant_steps": bound >> t, "parity": parity, "paths": r}
    results["parity"] = parity_all
    print("composition t=16 bound 2^20 n 2^16: call %.2f ms, composition %.1f ms, parity %s" % (
        r["ed_dlog"]["median_ms"], r["add_to_affine_download_numpy_lookup"]["median_ms"], parity), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1, default=float)
    eng.close()


if __name__ == "__main__":
    main()
