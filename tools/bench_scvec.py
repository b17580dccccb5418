#!/usr/bin/env python3
"""Scalar vector ops (zc_sc_sum_rows, zc_sc_dot_rows, zc_sc_powers) against the compositions they replace and against the bytes
they move, device-resident, the competing paths alternated in one process.  Writes profiles/r23_scvec.json.

Per shape: WARMUP untimed rounds, then REPEATS rounds in which every path runs once, one after the other; a sample is the wall
time between two device synchronisations of as many back-to-back calls as fill about 5 ms (at most 32), divided by their number
(a path that downloads synchronises itself in every call).  Reported per path: median, minimum, maximum and
spread = (max - min) / median of the samples; per baseline `new_over_this`, the ratio of the medians (above 1: the new call is
slower).  Every shape is checked first: the paths agree limb for limb.

Baselines
  muladd_chain_presplit / add_chain_presplit   a loop of zc_sc_muladd (zc_sc_add) over columns that are ALREADY split per term,
                        which a caller holding row-major records would first have to produce: this favours the composition.
  mul_download_host_sum zc_sc_mul of all records, the products downloaded and summed per row with numpy object integers (timed
                        up to 2^21 records; above that it is skipped and said so).
  pow_per_column        zc_sc_pow per column j with the exponent j, into columns split per term.
  bytes at the zc_sc_add rate: the bytes the call must move (inputs once, outputs once) divided by the rate zc_sc_add reaches at
                        2^24 rows in the same run (120 bytes per row); `over_bytes_bound` is the call's time over that bound.
The dot product's chained form (a build with -DZC_SCV_DOT_CHAINED=1, `--ab-lib`) runs beside the product on a second context."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP, REPEATS, SLOW_REPEATS = 3, 9, 3
L = (1 << 249) + 14490550575682688738086195780655237219
HOST_SUM_MAX = 1 << 21


def main():
    import torch
    import dusk_zerocaf_amd as z
    from dusk_zerocaf_amd import _lib
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_scvec.json"))
    ap.add_argument("--max-log2", type=int, default=24)
    ap.add_argument("--ab-lib", default=None, help="a second build of the library (python -m dusk_zerocaf_amd.build --variant NAME ZC_SCV_DOT_CHAINED=1)")
    args = ap.parse_args()
    eng = z.Engine()
    other = z.Engine(lib=_lib._bind(args.ab_lib)) if args.ab_lib else None
    rng = np.random.default_rng(23)
    i64 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()
    u64 = lambda t: t.cpu().numpy().view(np.uint64)

    def sync():
        torch.cuda.synchronize()
        eng.synchronize()
        if other:
            other.synchronize()

    def scalars(*shape):
        k = rng.integers(0, 1 << 52, size=shape + (5,), dtype=np.uint64)
        k[..., 4] &= np.uint64((1 << 40) - 1)
        return i64(k)

    def measure(paths, new, slow=()):
        """slow: paths that take seconds on the host (one warm-up call, SLOW_REPEATS samples)"""
        for i in range(WARMUP):
            for name, fn in paths.items():
                if i == 0 or name not in slow:
                    fn()
        sync()
        inner = {}
        for name, fn in paths.items():
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            inner[name] = int(min(32, max(1, 5e-3 / (time.perf_counter() - t0))))
        samples = {name: [] for name in paths}
        for i in range(REPEATS):
            for name, fn in paths.items():
                if name in slow and i >= SLOW_REPEATS:
                    continue
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
            if name != new:
                out[name]["new_over_this"] = out[new]["median_ms"] / out[name]["median_ms"]
        return out

    def host_values(t):
        a = u64(t)
        v = np.zeros(a.shape[:-1], dtype=object)
        for i in range(5):
            v = v + (a[..., i].astype(object) << (52 * i))
        return v

    same = lambda a, b: bool(torch.equal(a, b))
    results = {"tool": "tools/bench_scvec.py", "device": torch.cuda.get_device_name(0), "warmup": WARMUP, "repeats": REPEATS, "slow_repeats": SLOW_REPEATS, "shapes": []}
    # the rate of zc_sc_add at 2^24 rows: 120 bytes per row
    m = 1 << min(24, args.max_log2)
    x, y = scalars(m), scalars(m)
    r = measure({"sc_add": lambda: eng.sc_add(x, y), "sc_mul": lambda: eng.sc_mul(x, y)}, "sc_add")
    rate = m * 120 / r["sc_add"]["median_ms"] / 1e6                                     # GB/s
    results["sc_add"] = {"n": m, "GB_per_s": rate, "paths": r}
    print("zc_sc_add 2^%d: %.3f ms, %.0f GB/s; zc_sc_mul %.3f ms" % (m.bit_length() - 1, r["sc_add"]["median_ms"], rate, r["sc_mul"]["median_ms"]), flush=True)
    del x, y
    shapes = [(1 << 20, 2), (1 << 20, 8), (1 << 20, 64), (1, 1 << 20), (1, 1 << 24)]
    parity_all = True
    for n, t in shapes:
        if n * t > 1 << (args.max_log2 + 2):
            continue
        a, b = scalars(n, t), scalars(n, t)
        flat_a, flat_b = a.reshape(n * t, 5), b.reshape(n * t, 5)
        zero = i64(np.zeros((n, 5), dtype=np.uint64))
        for op in ("dot", "sum"):
            new = "sc_%s_rows" % op
            paths = {new: (lambda: eng.sc_dot_rows(a, b)) if op == "dot" else (lambda: eng.sc_sum_rows(a))}
            parity = True
            if t <= 64:
                ca, cb = [a[:, j].contiguous() for j in range(t)], [b[:, j].contiguous() for j in range(t)]

                def chain():
                    acc = zero
                    for j in range(t):
                        acc = eng.sc_muladd(ca[j], cb[j], acc) if op == "dot" else eng.sc_add(ca[j], acc)
                    return acc
                paths["muladd_chain_presplit" if op == "dot" else "add_chain_presplit"] = chain
                parity = parity and same(paths[new](), chain())
            if op == "dot" and n * t <= HOST_SUM_MAX:
                def host_sum():
                    v = host_values(eng.sc_mul(flat_a, flat_b)).reshape(n, t).sum(axis=1)
                    return [int(s) % L for s in v]
                paths["mul_download_host_sum"] = host_sum
                got = host_values(paths[new]())
                parity = parity and [int(g) for g in got] == host_sum()
            if op == "dot" and other:
                paths["dot_chained_variant"] = lambda: other.sc_dot_rows(a, b)
                parity = parity and same(paths[new](), paths["dot_chained_variant"]())
            if op == "dot" and t > 64:                                                  # one long row: against the sum of the products
                parity = parity and same(paths[new](), eng.sc_sum_rows(eng.sc_mul(flat_a, flat_b).reshape(n, t, 5)))
            r = measure(paths, new, slow=("mul_download_host_sum",))
            moved = n * t * (80 if op == "dot" else 40) + n * 40
            bound = moved / rate / 1e6
            entry = {"call": new, "n": n, "terms": t, "parity": bool(parity), "bytes_moved": moved, "bytes_bound_ms": bound, "over_bytes_bound": r[new]["median_ms"] / bound,
                     "GB_per_s": moved / r[new]["median_ms"] / 1e6, "paths": r}
            if op == "dot" and n * t > HOST_SUM_MAX:
                entry["skipped"] = ["mul_download_host_sum: more than 2^21 records of host integers"]
            results["shapes"].append(entry)
            parity_all = parity_all and bool(parity)
            print("%s %d x %d: %.3f ms (%.2f x the bytes bound), parity %s" % (new, n, t, r[new]["median_ms"], entry["over_bytes_bound"], parity), flush=True)
            if t <= 64:
                del ca, cb
        if (n, t) == (1 << 20, 8):                                                      # the shared b
            row = b[0].contiguous()
            tiled = row.unsqueeze(0).expand(n, t, 5).contiguous()
            paths = {"sc_dot_rows_shared_b": lambda: eng.sc_dot_rows(a, row, shared_b=True), "sc_dot_rows_tiled_b": lambda: eng.sc_dot_rows(a, tiled)}
            parity = same(paths["sc_dot_rows_shared_b"](), paths["sc_dot_rows_tiled_b"]())
            r = measure(paths, "sc_dot_rows_shared_b")
            moved = n * t * 40 + t * 40 + n * 40
            bound = moved / rate / 1e6
            results["shapes"].append({"call": "sc_dot_rows_shared_b", "n": n, "terms": t, "parity": bool(parity), "bytes_moved": moved, "bytes_bound_ms": bound,
                                      "over_bytes_bound": r["sc_dot_rows_shared_b"]["median_ms"] / bound, "GB_per_s": moved / r["sc_dot_rows_shared_b"]["median_ms"] / 1e6, "paths": r})
            parity_all = parity_all and bool(parity)
            print("shared b %d x %d: %.3f ms, parity %s" % (n, t, r["sc_dot_rows_shared_b"]["median_ms"], parity), flush=True)
            del row, tiled
        del a, b, flat_a, flat_b, zero
    # powers
    for n, t in ((1 << 20, 8), (1, 1 << 24)):
        if n * t > 1 << args.max_log2:
            continue
        x = scalars(n)
        paths = {"sc_powers": lambda: eng.sc_powers(x, t)}
        parity = True
        if t <= 64:
            exps = [i64(np.tile(np.array([j, 0, 0, 0, 0], dtype=np.uint64), (n, 1))) for j in range(t)]
            paths["pow_per_column"] = lambda: [eng.sc_pow(x, e) for e in exps]
            got = paths["sc_powers"]()
            parity = all(same(got[:, j].contiguous(), c) for j, c in enumerate(paths["pow_per_column"]()))
        else:                                                                           # one row: a sample of exponents against zc_sc_pow
            js = [0, 1, 2, 255, 256, 65535, 65536, 65537, t - 1]
            got = paths["sc_powers"]()
            e = i64(np.array([[j, 0, 0, 0, 0] for j in js], dtype=np.uint64))
            parity = same(got[0, js].contiguous(), eng.sc_pow(x.expand(len(js), 5).contiguous(), e))
        r = measure(paths, "sc_powers")
        moved = n * 40 + n * t * 40
        bound = moved / rate / 1e6
        results["shapes"].append({"call": "sc_powers", "n": n, "terms": t, "parity": bool(parity), "bytes_moved": moved, "bytes_bound_ms": bound,
                                  "over_bytes_bound": r["sc_powers"]["median_ms"] / bound, "GB_per_s": moved / r["sc_powers"]["median_ms"] / 1e6, "paths": r})
        parity_all = parity_all and bool(parity)
        print("sc_powers %d x %d: %.3f ms (%.2f x the bytes bound), parity %s" % (n, t, r["sc_powers"]["median_ms"], results["shapes"][-1]["over_bytes_bound"], parity), flush=True)
        del x
    results["parity"] = bool(parity_all)
    results["ab_lib"] = os.path.basename(args.ab_lib) if args.ab_lib else None
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1, default=float)
    eng.close()
    if other:
        other.close()


if __name__ == "__main__":
    main()
