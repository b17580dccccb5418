#!/usr/bin/env python3
"""Fixed-base MSM against zc_msm on the same pairs, device-resident scalars, one JSON record.

For every (n, batch): the table build (time, bytes, plan), then `--reps` timed rounds after `--warmup`, each round one
zc_msm_fixed call over the batch and `batch` zc_msm calls on the same pairs, alternated in this process; every timed
output is checked against zc_msm's with ed_eq.  Useful fraction = non-zero digits x 7 multiplications x 135 v_mad_u64_u32
over the 39.32 T lane-ops/s line of the zc_msm roofline (bench.py).  `--sweep n1,n2,..` times every window width 5..22 at
batch 1 (auto choice marked) instead.
Usage: python tools/bench_msm_fixed.py [--sizes 12:64,16:8,20:1,20:4,21:1] [--reps 20] [--warmup 3] [--out FILE]
       python tools/bench_msm_fixed.py --sweep 12,16,20 [--cs 5-22] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dusk_zerocaf_amd as z  # noqa: E402
from tests.vectors import rand_scalars_np  # noqa: E402

ROOF_T = 39.32e12            # v_mad_u64_u32 lane-ops/s: the line bench.py's zc_msm roofline uses
MADS_PER_MUL = 135
MULS_PER_ADD = 7             # mixed addition against an affine record


def nonzero_digits(K, c):
    """Non-zero signed c-bit digits of the scalars (k_msm_digits' recoding; the random scalars here are < 2^252)."""
    K = K.reshape(-1, 5).astype(np.uint64)
    W = -(-261 // c)
    half = 1 << (c - 1)
    carry = np.zeros(len(K), dtype=np.int64)
    nz = 0
    for w in range(W):
        bit = w * c
        idx, sh = bit // 52, bit % 52
        raw = np.zeros(len(K), dtype=np.uint64)
        if idx < 5:
            raw = K[:, idx] >> np.uint64(sh)
            if sh + c > 52 and idx + 1 < 5:
                raw |= K[:, idx + 1] << np.uint64(52 - sh)
            raw &= np.uint64((1 << c) - 1)
        r = raw.astype(np.int64) + carry
        carry = (r > half).astype(np.int64)
        d = r - carry * (1 << c)
        nz += int(np.count_nonzero(d))
    return nz


def sync_ms(f):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, r


def one_size(eng, lg, batch, reps, warmup, seed):
    n = 1 << lg
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()
    P = eng.ed_mul_base(dev(rand_scalars_np(n, seed, 249)))
    Kh = np.stack([rand_scalars_np(n, seed + 1 + b, 252) for b in range(batch)])
    K = dev(Kh)
    Kv = [K[b] for b in range(batch)]
    build_ms, tb = sync_ms(lambda: eng.msm_bases(P))
    plan = tb.plan
    rec = {"n": n, "batch": batch, "plan": plan, "table_build_ms": round(build_ms, 3),
           "table_bytes": n * plan["windows"] * plan["record_stride"], "zc_msm_plan": eng.msm_plan(n)}
    for _ in range(warmup):
        tb.msm(K)
        for b in range(batch):
            eng.msm(P, Kv[b])
    tf, tm, bad = [], [], 0
    for _ in range(reps):
        ms, got = sync_ms(lambda: tb.msm(K))
        tf.append(ms)
        ms, want = sync_ms(lambda: [eng.msm(P, Kv[b]) for b in range(batch)])
        tm.append(ms)
        bad += int(sum(eng.ed_eq(got[b:b + 1], want[b])[0] != 1 for b in range(batch)))
    tb.close()
    med = lambda v: float(np.median(v))
    useful = nonzero_digits(Kh, plan["window_bits"]) * MULS_PER_ADD * MADS_PER_MUL
    rec.update({
        "fixed_ms_per_call": round(med(tf), 4), "fixed_ms_min": round(min(tf), 4),
        "zc_msm_ms_for_batch": round(med(tm), 4), "zc_msm_ms_min": round(min(tm), 4),
        "fixed_pairs_per_s": round(batch * n / (med(tf) / 1e3)), "zc_msm_pairs_per_s": round(batch * n / (med(tm) / 1e3)),
        "speedup_vs_zc_msm": round(med(tm) / med(tf), 3),
        "fixed_useful_fraction": round(useful / (med(tf) / 1e3) / ROOF_T, 4),
        "mismatches": bad, "reps": reps})
    return rec


def sweep(eng, lgs, cs, reps):
    out = []
    for lg in lgs:
        n = 1 << lg
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()
        P = eng.ed_mul_base(dev(rand_scalars_np(n, 21, 249)))
        K = dev(rand_scalars_np(n, 22, 252))
        auto = eng.msm_fixed_plan(n)["window_bits"]
        row = {"n": n, "auto_c": auto, "ms": {}}
        for c in cs:
            if n * 128 * -(-261 // c) > (24 << 30):
                continue
            build_ms, tb = sync_ms(lambda: eng.msm_bases(P, window_bits=c))
            tb.msm(K)
            ts = [sync_ms(lambda: tb.msm(K))[0] for _ in range(reps)]
            tb.close()
            row["ms"][c] = round(float(np.median(ts)), 4)
            print("sweep n=2^%d c=%d: %.3f ms (build %.1f ms)" % (lg, c, row["ms"][c], build_ms), file=sys.stderr, flush=True)
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="12:64,16:8,20:1,20:4,21:1")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sweep", default="")
    ap.add_argument("--cs", default="5-22")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    eng = z.Engine()
    rec = {"lib": eng.lib.zc_version().decode(), "device": torch.cuda.get_device_name(0)}
    if a.sweep:
        lo, hi = (int(x) for x in a.cs.split("-"))
        rec["sweep"] = sweep(eng, [int(x) for x in a.sweep.split(",")], range(lo, hi + 1), max(3, a.reps))
    else:
        rec["sizes"] = []
        for i, s in enumerate(a.sizes.split(",")):
            lg, batch = (int(x) for x in s.split(":"))
            r = one_size(eng, lg, batch, a.reps, a.warmup, 1000 + 10 * i)
            print(json.dumps(r), file=sys.stderr, flush=True)
            rec["sizes"].append(r)
    eng.close()
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    return 0 if all(r.get("mismatches", 0) == 0 for r in rec.get("sizes", [])) else 1


if __name__ == "__main__":
    sys.exit(main())
