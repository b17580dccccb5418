#!/usr/bin/env python3
"""Batched variable-base MSM (zc_msm_batch) against one zc_msm call per instance, device-resident inputs, one JSON record.

For every (n, batch): `--reps` timed rounds after `--warmup`, each round one zc_msm_batch call over the batch and the same
instances as zc_msm calls, alternated in this process; every timed output row that zc_msm also computed is checked against it
with ed_eq.  Batches of more than --loop-max instances time zc_msm on the first --loop-max instances only and scale the time
by batch / loop-max (the record says so: "zc_msm_scaled_from").  Rates: pairs/s and instances/s.  Useful fraction, bucket
regime: non-zero digits x 7 (affine records; projective: 8) multiplications x 135 v_mad_u64_u32 over the 39.32 T lane-ops/s
line of the zc_msm roofline (bench.py); small-instance regime: the strict scalar multiplications' unified additions (bit
length + popcount - 1 per scalar) x 9 multiplications x 135 over the same line, and the time of zc_ed_scalar_mul alone on the
same pairs.
`--sweep`: (1) every window width c at the --sweep-c shapes (ZC_MSM_WINDOW=c, read at context creation); (2) the crossover:
at 2^20 pairs in all, n = 1, 2, 4, .., 2^14, both regimes, each forced by a build variant (build/variants/batch_buckets.so,
batch_scalarmul.so: ZC_MSM_BATCH_BUCKET_MIN_N = 1 / 2^30, built by this tool when missing) run in a child process.
Usage: python tools/bench_msm_batch.py [--sizes 12:64,16:8,14:16,1:262144,12:1,16:1] [--reps 10] [--warmup 2] [--out FILE]
       python tools/bench_msm_batch.py --sweep [--sweep-c 12:64,10:256,14:16,8:1024] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dusk_zerocaf_amd as z  # noqa: E402
from tests.vectors import rand_scalars_np  # noqa: E402
from tools.bench_msm_fixed import nonzero_digits, sync_ms, ROOF_T, MADS_PER_MUL  # noqa: E402

VARIANTS = {"buckets": "ZC_MSM_BATCH_BUCKET_MIN_N=1", "scalar_mul": "ZC_MSM_BATCH_BUCKET_MIN_N=1073741824"}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def inputs(eng, n, batch, seed):
    P = eng.ed_mul_base(dev(rand_scalars_np(n * batch, seed, 249))).view(batch, n, 20)
    Kh = rand_scalars_np(n * batch, seed + 1, 252).reshape(batch, n, 5)
    return P, Kh, dev(Kh)


def addition_count(Kh):
    """Unified additions of the strict double-and-add over these (< 2^252) scalars: bit length + popcount - 1 each."""
    K = Kh.reshape(-1, 5)
    v = [int(K[i, 0]) | int(K[i, 1]) << 52 | int(K[i, 2]) << 104 | int(K[i, 3]) << 156 | int(K[i, 4]) << 208 for i in range(len(K))]
    return sum(x.bit_length() + bin(x).count("1") - 1 for x in v if x)


def one_size(eng, n, batch, reps, warmup, loop_max, seed):
    P, Kh, K = inputs(eng, n, batch, seed)
    plan = eng.msm_batch_plan(n, batch)
    sub = min(batch, loop_max)
    rec = {"n": n, "batch": batch, "pairs": n * batch, "plan": plan}
    if sub < batch:
        rec["zc_msm_scaled_from"] = sub
    for _ in range(warmup):
        eng.msm_batch(P, K)
        for b in range(sub):
            eng.msm(P[b], K[b])
    tb, tm, bad = [], [], 0
    for _ in range(reps):
        ms, got = sync_ms(lambda: eng.msm_batch(P, K))
        tb.append(ms)
        ms, want = sync_ms(lambda: [eng.msm(P[b], K[b]) for b in range(sub)])
        tm.append(ms * batch / sub)
        bad += int(sum(eng.ed_eq(got[b:b + 1], want[b])[0] != 1 for b in range(sub)))
    med = lambda v: float(np.median(v))
    t = med(tb) / 1e3
    rec.update({"batch_ms_per_call": round(med(tb), 4), "batch_ms_min": round(min(tb), 4),
                "zc_msm_ms_for_batch": round(med(tm), 4), "speedup_vs_zc_msm": round(med(tm) / med(tb), 3),
                "pairs_per_s": round(n * batch / t), "instances_per_s": round(batch / t),
                "mismatches": bad, "checked_rows_per_rep": sub, "reps": reps})
    if plan["regime"] == "buckets":
        muls = 7 if plan["affine"] else 8
        rec["useful_fraction"] = round(nonzero_digits(Kh, plan["window_bits"]) * muls * MADS_PER_MUL / t / ROOF_T, 4)
    else:
        rec["useful_fraction"] = round(addition_count(Kh) * 9 * MADS_PER_MUL / t / ROOF_T, 4)
        Pf, Kf = P.reshape(-1, 20), K.reshape(-1, 5)
        eng.ed_scalar_mul(Pf, Kf)
        ts = [sync_ms(lambda: eng.ed_scalar_mul(Pf, Kf))[0] for _ in range(reps)]
        rec["ed_scalar_mul_ms_same_pairs"] = round(med(ts), 4)
        rec["batch_over_scalar_mul"] = round(med(tb) / med(ts), 3)
    return rec


def time_batch(eng, n, batch, reps, seed):
    P, _, K = inputs(eng, n, batch, seed)
    eng.msm_batch(P, K)
    return round(float(np.median([sync_ms(lambda: eng.msm_batch(P, K))[0] for _ in range(reps)])), 4)


def sweep_c(shapes, reps):
    out = []
    for n, batch in shapes:
        auto = None
        row = {"n": n, "batch": batch, "ms": {}}
        for c in range(5, 15):
            os.environ["ZC_MSM_WINDOW"] = str(c)
            eng = z.Engine()
            os.environ.pop("ZC_MSM_WINDOW")
            row["ms"][c] = time_batch(eng, n, batch, reps, 31)
            eng.close()
            print("sweep c: n=%d batch=%d c=%d %.3f ms" % (n, batch, c, row["ms"][c]), file=sys.stderr, flush=True)
        eng = z.Engine()
        auto = eng.msm_batch_plan(n, batch)["window_bits"]
        eng.close()
        row["auto_c"] = auto
        row["best_c"] = min(row["ms"], key=row["ms"].get)
        out.append(row)
    return out


def regime_child(reps):
    """(in a child process on one build variant) 2^20 pairs in all, n = 1 .. 2^14"""
    eng = z.Engine()
    rows = {}
    for lg in range(0, 15):
        n = 1 << lg
        batch = (1 << 20) // n
        plan = eng.msm_batch_plan(n, batch)
        if plan["regime"] == "buckets" and batch * plan["windows"] << (plan["window_bits"] - 1) > (96 << 20):
            rows[n] = None                                      # > 96 M buckets (14 GB of bucket records): not run
            continue
        rows[n] = time_batch(eng, n, batch, reps, 41)
        print("regime %s: n=%d batch=%d %s ms" % (plan["regime"], n, batch, rows[n]), file=sys.stderr, flush=True)
    eng.close()
    print(json.dumps(rows))


def sweep_regimes(reps):
    from dusk_zerocaf_amd import build
    res = {}
    for name, define in VARIANTS.items():
        lib = os.path.join(ROOT, "build", "variants", "batch_%s.so" % name.replace("_", ""))
        if not os.path.exists(lib):
            lib = build.build_variant("batch_%s" % name.replace("_", ""), [define])
        env = dict(os.environ, ZC_LIB_PATH=lib)
        outp = subprocess.run([sys.executable, os.path.abspath(__file__), "--regime-child", "--reps", str(reps)], env=env,
                              stdout=subprocess.PIPE, text=True, timeout=900, check=True).stdout
        res[name] = {int(k): v for k, v in json.loads(outp.strip().splitlines()[-1]).items()}
    rows = []
    for n in sorted(res["buckets"]):
        b, s = res["buckets"][n], res["scalar_mul"][n]
        rows.append({"n": n, "batch": (1 << 20) // n, "buckets_ms": b, "scalar_mul_ms": s,
                     "faster": None if b is None else ("buckets" if b < s else "scalar_mul")})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="12:64,16:8,14:16,1:262144,12:1,16:1")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop-max", type=int, default=256)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--sweep-c", default="12:64,10:256,14:16,8:1024")
    ap.add_argument("--regime-child", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.regime_child:
        regime_child(max(3, a.reps))
        return 0
    eng = z.Engine()
    rec = {"lib": eng.lib.zc_version().decode(), "device": torch.cuda.get_device_name(0)}
    eng.close()
    if a.sweep:
        shapes = [tuple(1 << int(x) if i == 0 else int(x) for i, x in enumerate(s.split(":"))) for s in a.sweep_c.split(",")]
        rec["sweep_c"] = sweep_c(shapes, max(3, a.reps))
        rec["sweep_regimes_2_20_pairs"] = sweep_regimes(max(3, a.reps))
    else:
        eng = z.Engine()
        rec["sizes"] = []
        for i, s in enumerate(a.sizes.split(",")):
            lg, batch = (int(x) for x in s.split(":"))
            r = one_size(eng, 1 << lg, batch, a.reps, a.warmup, a.loop_max, 2000 + 10 * i)
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
