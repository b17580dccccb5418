#!/usr/bin/env python3
"""Point sums (zc_ed_sum_rows, zc_ris_sum_rows) against the compositions they replace, device-resident, the competing paths
alternated in one process.  Writes profiles/r21_sum_rows.json.

Per shape: WARMUP untimed rounds, then REPEATS rounds in which every path runs once, one after the other; a sample is the wall
time between two device synchronisations of as many back-to-back calls as fill about 5 ms (at most 32), divided by their number
(zc_msm and zc_msm_batch return host arrays and synchronise themselves in every call).
Reported per path: median, minimum, maximum and spread = (max - min) / median of the samples; per baseline the ratio of the
medians.  Every shape is checked first: the paths agree as group elements (zc_ed_eq) or byte for byte (wire form).

The pairwise baseline of the short rows gets its terms in arrays already split per term, which a caller holding row-major
records would first have to produce: this favours the composition."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP, REPEATS = 3, 9


def main():
    import torch
    import dusk_zerocaf_amd as z
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_sum_rows.json"))
    ap.add_argument("--max-log2", type=int, default=24)
    args = ap.parse_args()
    eng = z.Engine()
    rng = np.random.default_rng(21)
    i64 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()

    def sync():
        torch.cuda.synchronize()
        eng.synchronize()

    def points(n):
        """n valid points on the device: 2^20 distinct multiples of the basepoint, tiled."""
        m = min(n, 1 << 20)
        k = rng.integers(0, 1 << 52, size=(m, 5), dtype=np.uint64)
        k[:, 4] &= np.uint64((1 << 44) - 1)
        p = eng.ed_mul_base(i64(k))
        return p if m == n else p.repeat(n // m, 1).contiguous()

    def measure(paths):
        for _ in range(WARMUP):
            for fn in paths.values():
                fn()
        sync()
        # calls per sample: enough to fill about 5 ms, so that one launch and one synchronisation weigh little in a sample
        inner = {}
        for name, fn in paths.items():
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            inner[name] = int(min(32, max(1, 5e-3 / (time.perf_counter() - t0))))
        samples = {name: [] for name in paths}
        for _ in range(REPEATS):
            for name, fn in paths.items():
                sync()
                t0 = time.perf_counter()
                for _ in range(inner[name]):
                    fn()
                sync()
                samples[name].append((time.perf_counter() - t0) * 1e3 / inner[name])
        out = {}
        for name, s in samples.items():
            med = float(np.median(s))
            out[name] = {"median_ms": med, "min_ms": min(s), "max_ms": max(s), "spread": (max(s) - min(s)) / med, "calls_per_sample": inner[name], "samples_ms": s}
        for name in out:
            if name != "sum_rows":
                out[name]["sum_rows_over_this"] = out["sum_rows"]["median_ms"] / out[name]["median_ms"]
        return out

    one = lambda *shape: i64(np.tile(np.array([1, 0, 0, 0, 0], dtype=np.uint64), shape + (1,)))
    same = lambda a, b: bool(eng.ed_eq(a.reshape(-1, 20), b.reshape(-1, 20)).cpu().numpy().all())
    dev_row = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()

    def halving(p):
        while p.shape[0] > 1:
            h = p.shape[0] // 2
            p = eng.ed_add(p[:h], p[h:2 * h])
        return p

    results = {"tool": "tools/bench_sum_rows.py", "device": torch.cuda.get_device_name(0), "warmup": WARMUP, "repeats": REPEATS, "shapes": []}
    # 2^20 rows x 2 / 4 / 8 terms
    n = 1 << 20
    for t in (2, 4, 8):
        p = points(n * t).reshape(n, t, 20)
        split = [p[:, j].contiguous() for j in range(t)]
        k = one(n, t)

        def pairwise():
            acc = eng.ed_add(split[0], split[1])
            for j in range(2, t):
                acc = eng.ed_add(acc, split[j])
            return acc
        paths = {"sum_rows": lambda: eng.ed_sum_rows(p), "ed_add_pairwise_presplit": pairwise, "ed_lincomb_unit_scalars": lambda: eng.ed_lincomb(p, k)}
        parity = np.array_equal(paths["sum_rows"]().cpu().numpy(), pairwise().cpu().numpy()) and same(paths["sum_rows"](), paths["ed_lincomb_unit_scalars"]())
        r = measure(paths)
        results["shapes"].append({"form": "edwards", "n": n, "terms": t, "parity": parity, "G_additions_per_s": n * (t - 1) / r["sum_rows"]["median_ms"] / 1e6, "paths": r})
        print("ed %d x %d: %.3f ms, parity %s" % (n, t, r["sum_rows"]["median_ms"], parity), flush=True)
        del p, split, k
    # one row
    for lg in (16, 20, 24):
        if lg > args.max_log2:
            continue
        m = 1 << lg
        p = points(m)
        k = one(m)
        row = p.reshape(1, m, 20)
        paths = {"sum_rows": lambda: eng.ed_sum_rows(row), "msm_unit_scalars": lambda: eng.msm(p, k), "ed_add_halving_loop": lambda: halving(p)}
        parity = same(paths["sum_rows"](), halving(p)) and same(paths["sum_rows"](), dev_row(eng.msm(p, k)))
        r = measure(paths)
        results["shapes"].append({"form": "edwards", "n": 1, "terms": m, "parity": parity, "G_additions_per_s": (m - 1) / r["sum_rows"]["median_ms"] / 1e6,
                                  "GB_per_s": m * 160 / r["sum_rows"]["median_ms"] / 1e6, "paths": r})
        print("ed 1 x 2^%d: %.3f ms, parity %s" % (lg, r["sum_rows"]["median_ms"], parity), flush=True)
        del p, k, row
    # 1024 x 1024
    p = points(1 << 20).reshape(1024, 1024, 20)
    k = one(1024, 1024)
    paths = {"sum_rows": lambda: eng.ed_sum_rows(p), "msm_batch_unit_scalars": lambda: eng.msm_batch(p, k)}
    parity = same(paths["sum_rows"](), dev_row(eng.msm_batch(p, k)))
    r = measure(paths)
    results["shapes"].append({"form": "edwards", "n": 1024, "terms": 1024, "parity": parity, "paths": r})
    print("ed 1024 x 1024: %.3f ms, parity %s" % (r["sum_rows"]["median_ms"], parity), flush=True)
    # wire form
    for n, t in ((1 << 20, 2), (1, 1 << 20)):
        pts = points(n * t)
        enc = eng.ris_compress(eng.ed_double(pts)).reshape(n, t, 32).contiguous()
        del pts

        def composed():
            q, _ = eng.ris_decompress(enc.reshape(n * t, 32))
            return eng.ris_compress(eng.ed_sum_rows(q.reshape(n, t, 20)))
        paths = {"sum_rows": lambda: eng.ris_sum_rows(enc), "decompress_sum_compress": composed}
        if t <= 8:
            k = one(n, t)
            paths["ris_lincomb_unit_scalars"] = lambda: eng.ris_lincomb(enc, k)
        got = paths["sum_rows"]()[0].cpu().numpy()
        parity = np.array_equal(got, composed().cpu().numpy()) and (t > 8 or np.array_equal(got, paths["ris_lincomb_unit_scalars"]()[0].cpu().numpy()))
        r = measure(paths)
        results["shapes"].append({"form": "wire", "n": n, "terms": t, "parity": bool(parity), "paths": r})
        print("wire %d x %d: %.3f ms, parity %s" % (n, t, r["sum_rows"]["median_ms"], parity), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1, default=float)
    eng.close()


if __name__ == "__main__":
    main()
