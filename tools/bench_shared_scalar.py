#!/usr/bin/env python3
"""One scalar for a whole batch: the two shared-scalar calls against the calls they replace, one JSON record.

Device-resident inputs, HIP events on the context's stream.  Per pair and size both sides are warmed up, then timed one after
the other in every one of `--reps` rounds (alternated in this process, at least five); a sample is `inner` back-to-back calls
between two events, `inner` chosen per side so that a sample lasts about 20 ms.  Every pair carries a `parity` flag from a
comparison of whole outputs in the same run (encodings for the Edwards form: the two calls return other representatives).
  * ed:    zc_ed_scalar_mul_shared(P, k)   |  zc_ed_scalar_mul(P, k in every row, ZC_SCALAR_MUL_FAST)
  * wire:  zc_ris_mul_shared(E, k)         |  zc_ris_roundtrip_mul(E, k in every row)
The comparison is against the existing entry points, never against the new code itself.  k is one seeded scalar below L (a view
key); the points are seeded multiples of the basepoint, the encodings their Ristretto encodings.
Usage: python tools/bench_shared_scalar.py [--lgs 16,20,22] [--reps 7] [--warmup 2] [--out profiles/r18_shared_scalar.json]"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FAST = 16
POOL = 1 << 12                   # distinct points, made on the device; longer batches repeat them


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lgs", default="16,20,22")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.reps >= 5, "the two sides alternate at least five times"
    import torch
    import dusk_zerocaf_amd as z
    from oracle import pymodel as pm
    eng = z.Engine([0])
    st = torch.cuda.current_stream()
    eng.set_stream(st.cuda_stream)
    rng = np.random.default_rng(1800)
    rand_sc = lambda n: np.array([pm.limbs(int.from_bytes(rng.bytes(40), "little") % pm.L) for _ in range(n)], dtype=np.uint64)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64) if a.dtype != np.uint8 else np.ascontiguousarray(a)).cuda()
    pool_pts = eng.ed_mul_base(dev(rand_sc(POOL)))                              # (POOL, 20) on the device
    pool_enc = eng.ris_compress(pool_pts)
    k = rand_sc(1)[0]
    rec = {"lib": eng.lib.zc_version().decode(), "device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
           "scalar_bits": int(pm.from_limbs([int(x) for x in k])).bit_length(), "distinct_points": POOL, "sizes": []}
    ok = True
    for lg in [int(x) for x in args.lgs.split(",")]:
        n = 1 << lg
        idx = torch.arange(n, device="cuda") % POOL
        P, E = pool_pts[idx].contiguous(), pool_enc[idx].contiguous()
        K = dev(np.tile(k, (n, 1)))
        entry = {"lg_rows": lg, "rows": n}
        # the Edwards form
        a, b = eng.ed_scalar_mul_shared(P, k), eng.ed_scalar_mul(P, K, flags=FAST)
        parity = bool((eng.ed_compress(a)[0] == eng.ed_compress(b)[0]).all()) and bool(eng.ed_eq(a, b).all())
        del a, b
        pair = run_pair({"zc_ed_scalar_mul_shared": lambda: eng.ed_scalar_mul_shared(P, k), "zc_ed_scalar_mul_fast_replicated_k": lambda: eng.ed_scalar_mul(P, K, flags=FAST)},
                        args.reps, args.warmup, st)
        pair["parity"] = parity
        pair["ratio_shared_over_replaced"] = round(pair["zc_ed_scalar_mul_shared"]["median_ms"] / pair["zc_ed_scalar_mul_fast_replicated_k"]["median_ms"], 4)
        entry["ed"] = pair
        ok = ok and parity
        # the wire form
        (a, aok), (b, bok) = eng.ris_mul_shared(E, k), eng.ris_roundtrip_mul(E, K)
        parity = bool((a == b).all()) and bool((aok == bok).all()) and bool(aok.all())
        del a, b, aok, bok
        pair = run_pair({"zc_ris_mul_shared": lambda: eng.ris_mul_shared(E, k), "zc_ris_roundtrip_mul_replicated_k": lambda: eng.ris_roundtrip_mul(E, K)},
                        args.reps, args.warmup, st)
        pair["parity"] = parity
        pair["ratio_shared_over_replaced"] = round(pair["zc_ris_mul_shared"]["median_ms"] / pair["zc_ris_roundtrip_mul_replicated_k"]["median_ms"], 4)
        entry["wire"] = pair
        ok = ok and parity
        print("2^%d rows: ed %.4f (parity %s), wire %.4f (parity %s)" % (lg, entry["ed"]["ratio_shared_over_replaced"], entry["ed"]["parity"],
                                                                         entry["wire"]["ratio_shared_over_replaced"], entry["wire"]["parity"]), file=sys.stderr, flush=True)
        rec["sizes"].append(entry)
        del P, E, K, idx
        torch.cuda.empty_cache()
    at20 = [e for e in rec["sizes"] if e["lg_rows"] == 20]
    if at20:
        rec["ships"] = {form: at20[0][form]["ratio_shared_over_replaced"] <= 1.0 for form in ("ed", "wire")}       # the condition: not above at 2^20 rows
    eng.close()
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
