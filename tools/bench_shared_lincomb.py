#!/usr/bin/env python3
"""One scalar VECTOR for a whole batch: the two shared-scalar linear combinations against the calls they replace, one JSON record.

Device-resident inputs, HIP events on the context's stream.  Per pair both sides are warmed up, then timed one after the other
in every one of `--reps` rounds (alternated in this process, at least seven); a sample is `inner` back-to-back calls between two
events, `inner` chosen per side so that a sample lasts about 20 ms.  Every pair carries a `parity` flag from a comparison of
whole outputs in the same run (encodings for the Edwards form: the calls return other representatives) and the run-to-run
spread of either side.
  * ed (a):  zc_ed_lincomb_shared(P, k)   |  zc_ed_lincomb(P, k tiled into every row)
  * ed (b):  zc_ed_lincomb_shared(P, k)   |  terms x zc_ed_scalar_mul_shared + (terms - 1) x zc_ed_add
  * wire:    zc_ris_lincomb_shared(E, k)  |  zc_ris_lincomb(E, k tiled into every row, no base term)
The comparisons are against existing entry points, never against the new code itself.  `count_ratio` beside every measured
ratio is the ratio of field multiplications per row.  The scalars are seeded values below L; the points are seeded
multiples of the basepoint, the encodings their Ristretto encodings.
Usage: python tools/bench_shared_lincomb.py [--cases 20:2,20:4,18:8,16:2] [--reps 7] [--warmup 2] [--out profiles/r19_shared_lincomb.json]"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POOL = 1 << 12                   # distinct points, made on the device; longer batches repeat them
# field multiplications per row, by the count of DESIGN 4.9 (averages over 300 random 252-bit vectors per term count)
COUNT = {"shared": {1: 2224, 2: 2656, 4: 3538, 8: 5255}, "lincomb": lambda t: 1827 + 567 * t, "compose": lambda t: 2224 * t + 9 * (t - 1)}


def sample_ms(f, inner, st):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(inner):
        f()
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def run_pair(paths, reps, warmup, st):
    """paths: {name: callable}, two of them; the sides alternate in every round."""
    import torch
    inner = {}
    for name, f in paths.items():
        for _ in range(warmup):
            f()
        torch.cuda.synchronize()
        inner[name] = max(1, min(200, math.ceil(20.0 / max(sample_ms(f, 1, st), 1e-3))))
    times = {name: [] for name in paths}
    for _ in range(reps):
        for name, f in paths.items():
            times[name].append(sample_ms(f, inner[name], st))
    out = {}
    for name, v in times.items():
        med = float(np.median(v))
        out[name] = {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "spread": round((max(v) - min(v)) / med, 4),
                     "calls_per_sample": inner[name], "samples": len(v)}
    return out


def finish(pair, new, old, parity, count_ratio):
    pair["parity"] = parity
    pair["ratio_shared_over_replaced"] = round(pair[new]["median_ms"] / pair[old]["median_ms"], 4)
    pair["count_ratio"] = round(count_ratio, 4) if count_ratio else None
    pair["spread"] = max(pair[new]["spread"], pair[old]["spread"])
    pair["below_by_more_than_the_spread"] = pair["ratio_shared_over_replaced"] < 1.0 - pair["spread"]
    return pair


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="20:2,20:4,18:8,16:2", help="lg(rows):terms, comma-separated")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.reps >= 7, "the two sides alternate at least seven times"
    import torch
    import dusk_zerocaf_amd as z
    from oracle import pymodel as pm
    eng = z.Engine([0])
    st = torch.cuda.current_stream()
    eng.set_stream(st.cuda_stream)
    rng = np.random.default_rng(1900)
    rand_sc = lambda n: np.array([pm.limbs(int.from_bytes(rng.bytes(40), "little") % pm.L) for _ in range(n)], dtype=np.uint64)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64) if a.dtype != np.uint8 else np.ascontiguousarray(a)).cuda()
    pool_pts = eng.ed_mul_base(dev(rand_sc(POOL)))                              # (POOL, 20) on the device
    pool_enc = eng.ris_compress(pool_pts)
    rec = {"lib": eng.lib.zc_version().decode(), "device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
           "distinct_points": POOL, "cases": []}
    ok = True
    for case in args.cases.split(","):
        lg, t = [int(x) for x in case.split(":")]
        n = 1 << lg
        idx = (torch.arange(n * t, device="cuda") * 7 + 3) % POOL
        P, E = pool_pts[idx].reshape(n, t, 20).contiguous(), pool_enc[idx].reshape(n, t, 32).contiguous()
        k = rand_sc(t)
        K = dev(np.tile(k.reshape(1, t, 5), (n, 1, 1)))
        cols = [P[:, j].contiguous() for j in range(t)]
        entry = {"lg_rows": lg, "rows": n, "terms": t, "scalar_bits": [int(pm.from_limbs([int(x) for x in kj])).bit_length() for kj in k]}
        shared = lambda: eng.ed_lincomb_shared(P, k)
        tiled = lambda: eng.ed_lincomb(P, K)

        def compose():
            acc = eng.ed_scalar_mul_shared(cols[0], k[0])
            for j in range(1, t):
                acc = eng.ed_add(acc, eng.ed_scalar_mul_shared(cols[j], k[j]))
            return acc
        a, b, c = shared(), tiled(), compose()
        ea = eng.ed_compress(a)[0]
        parity = bool((ea == eng.ed_compress(b)[0]).all()) and bool((ea == eng.ed_compress(c)[0]).all()) and bool(eng.ed_eq(a, b).all())
        del a, b, c, ea
        cs = COUNT["shared"].get(t)
        pair = run_pair({"zc_ed_lincomb_shared": shared, "zc_ed_lincomb_tiled_k": tiled}, args.reps, args.warmup, st)
        entry["ed_vs_lincomb"] = finish(pair, "zc_ed_lincomb_shared", "zc_ed_lincomb_tiled_k", parity, cs and cs / COUNT["lincomb"](t))
        pair = run_pair({"zc_ed_lincomb_shared": shared, "scalar_mul_shared_and_add": compose}, args.reps, args.warmup, st)
        entry["ed_vs_composition"] = finish(pair, "zc_ed_lincomb_shared", "scalar_mul_shared_and_add", parity, cs and cs / COUNT["compose"](t))
        ok = ok and parity
        wshared = lambda: eng.ris_lincomb_shared(E, k)
        wtiled = lambda: eng.ris_lincomb(E, K)
        (a, aok), (b, bok) = wshared(), wtiled()
        parity = bool((a == b).all()) and bool((aok == bok).all()) and bool(aok.all())
        del a, b, aok, bok
        pair = run_pair({"zc_ris_lincomb_shared": wshared, "zc_ris_lincomb_tiled_k": wtiled}, args.reps, args.warmup, st)
        # both sides decode every term (about 265 each); the replaced call ends in ris_compress's power (about 250), this one in the fused double-and-encode (about 32)
        entry["wire_vs_ris_lincomb"] = finish(pair, "zc_ris_lincomb_shared", "zc_ris_lincomb_tiled_k", parity,
                                              cs and (cs + 265 * t + 32) / (COUNT["lincomb"](t) + 265 * t + 250))
        ok = ok and parity
        print("2^%d rows, %d terms: ed/lincomb %.4f, ed/composition %.4f, wire %.4f (parity %s)" % (
            lg, t, entry["ed_vs_lincomb"]["ratio_shared_over_replaced"], entry["ed_vs_composition"]["ratio_shared_over_replaced"],
            entry["wire_vs_ris_lincomb"]["ratio_shared_over_replaced"], parity and entry["ed_vs_lincomb"]["parity"]), file=sys.stderr, flush=True)
        rec["cases"].append(entry)
        del P, E, K, idx, cols
        torch.cuda.empty_cache()
    eng.close()
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
