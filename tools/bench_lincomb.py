#!/usr/bin/env python3
"""zc_ed_lincomb against the composition the library offered before it, device-resident, one JSON record.

For every shape (terms t, rows n): inputs on the device, every path warmed up, then `--reps` rounds in which the two paths
are timed one after the other (alternated in this process, host clock around a device synchronisation):
  * lincomb:      one Engine.ed_lincomb call;
  * composition:  t ed_scalar_mul(flags=FAST) calls on per-term views copied contiguous beforehand + t - 1 ed_add calls,
                  outputs left on the device.
Every output row of the two paths is compared with ed_eq on the device ("parity").  The two-term shape is also timed
against msm_batch(n=2) on 2^18 instances (whose OUTPUT is host memory and whose call is synchronous: a different
residency, the record says so), and t = 1 against the windowed multiplication itself, which is timed twice to give the
run-to-run spread.  Reported per path: median, min, max in ms, rows/s; the ratio of the medians; the field multiplications
per row the two algorithms need (1827 + 567 t against 2394 t + 9 (t - 1)) and the fraction of the multiplier roofline that
count reaches ("useful work"); the ring geometry the call used.
Usage: python tools/bench_lincomb.py [--shapes 2:20,4:20,8:20,4:18,8:18,1:20] [--reps 10] [--warmup 2] [--out profiles/r10_lincomb.json]
       python tools/bench_lincomb.py --profile-run    (one call per shape and path, for a kernel trace)"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dusk_zerocaf_amd as z  # noqa: E402
from tests.vectors import rand_scalars_np  # noqa: E402
from tools.bench_msm_fixed import sync_ms, ROOF_T, MADS_PER_MUL  # noqa: E402

FAST = 16
GATE = 1.3


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def muls_lincomb(t):
    return 1827 + 567 * t


def muls_composition(t):
    return 2394 * t + 9 * (t - 1)


def geometry(t):
    """The slot geometry zc_ed_lincomb uses for t terms (zerocaf_hip.hip: ring_units_per_xcd / fast_ring)."""
    units = 512 if t <= 1 else min(512 * t, 2048)
    block = 128 if t > 4 else 256
    return {"slot_units": t, "units_per_xcd": units, "slots_per_xcd": min(512, units // t), "table_MiB": units * 8 * 64 // 1024,
            "workgroup": block, "lds_bytes_per_workgroup": 36 * t * block + 16}


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def inputs(eng, t, n, seed):
    P = eng.ed_mul_base(dev(rand_scalars_np(n * t, seed, 249))).view(n, t, 20)
    K = dev(rand_scalars_np(n * t, seed + 1, 252).reshape(n, t, 5))
    cols = [(P[:, j].contiguous(), K[:, j].contiguous()) for j in range(t)]
    return P, K, cols


def compose(eng, cols):
    acc = None
    for p, k in cols:
        q = eng.ed_scalar_mul(p, k, flags=FAST)
        acc = q if acc is None else eng.ed_add(acc, q)
    return acc


def one_shape(eng, t, lg, reps, warmup, seed):
    n = 1 << lg
    P, K, cols = inputs(eng, t, n, seed)
    for _ in range(warmup):
        eng.ed_lincomb(P, K)
        compose(eng, cols)
    tl, tc, tc2, parity = [], [], [], True
    for _ in range(reps):
        ms, got = sync_ms(lambda: eng.ed_lincomb(P, K))
        tl.append(ms)
        ms, want = sync_ms(lambda: compose(eng, cols))
        tc.append(ms)
        if t == 1:                                              # the same call once more: the run-to-run spread
            tc2.append(sync_ms(lambda: compose(eng, cols))[0])
        parity = parity and bool(eng.ed_eq(got, want).all())
    ml, mc = float(np.median(tl)), float(np.median(tc))
    rec = {"terms": t, "rows": n, "reps": reps, "parity_every_row": parity, "lincomb": stats(tl), "composition": stats(tc),
           "composition_calls": "%d x ed_scalar_mul(FAST) + %d x ed_add" % (t, t - 1),
           "speedup_vs_composition": round(mc / ml, 3), "rows_per_s": round(n / (ml / 1e3)),
           "muls_per_row": {"lincomb": muls_lincomb(t), "composition": muls_composition(t),
                            "ratio": round(muls_composition(t) / muls_lincomb(t), 3)},
           "useful_fraction_of_multiplier_roof": round(n * muls_lincomb(t) * MADS_PER_MUL / (ml / 1e3) / ROOF_T, 4),
           "geometry": geometry(t)}
    if t == 1:
        rec["fast_again"] = stats(tc2)
        rec["fast_run_to_run_spread"] = round(abs(float(np.median(tc2)) - mc) / mc, 4)
        rec["lincomb_vs_fast"] = round(ml / mc, 4)
    if t == 2 and lg == 20:
        rec["gate"] = {"required_speedup": GATE, "met": bool(mc / ml >= GATE and parity)}
    return rec


def versus_msm_batch(eng, reps, warmup, seed):
    """t = 2 on 2^18 rows against msm_batch(n = 2) on the same instances.  msm_batch returns HOST memory and synchronises;
    ed_lincomb leaves its output on the device -- the two numbers include different things."""
    n, t = 1 << 18, 2
    P, K, _ = inputs(eng, t, n, seed)
    for _ in range(warmup):
        eng.ed_lincomb(P, K)
        eng.msm_batch(P, K)
    tl, tb, parity = [], [], True
    for _ in range(reps):
        ms, got = sync_ms(lambda: eng.ed_lincomb(P, K))
        tl.append(ms)
        ms, want = sync_ms(lambda: eng.msm_batch(P, K))
        tb.append(ms)
        parity = parity and bool(eng.ed_eq(got, dev(want)).all())
    return {"terms": t, "rows": n, "parity_every_row": parity, "lincomb": stats(tl), "msm_batch": stats(tb),
            "speedup_vs_msm_batch": round(float(np.median(tb)) / float(np.median(tl)), 3),
            "note": "msm_batch copies its results to pageable host memory inside the call; ed_lincomb's stay on the device"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2:20,4:20,8:20,4:18,8:18,1:20")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split(":")) for s in a.shapes.split(",")]
    eng = z.Engine()
    if a.profile_run:
        for i, (t, lg) in enumerate(shapes):
            P, K, cols = inputs(eng, t, 1 << lg, 3000 + 10 * i)
            for _ in range(2):
                eng.ed_lincomb(P, K)
                compose(eng, cols)
            torch.cuda.synchronize()
        eng.close()
        return 0
    rec = {"lib": eng.lib.zc_version().decode(), "device": torch.cuda.get_device_name(0), "shapes": []}
    for i, (t, lg) in enumerate(shapes):
        r = one_shape(eng, t, lg, a.reps, a.warmup, 3000 + 10 * i)
        print(json.dumps(r), file=sys.stderr, flush=True)
        rec["shapes"].append(r)
    rec["two_terms_vs_msm_batch"] = versus_msm_batch(eng, a.reps, a.warmup, 3900)
    print(json.dumps(rec["two_terms_vs_msm_batch"]), file=sys.stderr, flush=True)
    eng.close()
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    ok = all(r["parity_every_row"] for r in rec["shapes"]) and rec["two_terms_vs_msm_batch"]["parity_every_row"]
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
