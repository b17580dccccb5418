#!/usr/bin/env python3
"""zc_ris_double_and_compress against the composition it replaces, zc_ed_double then zc_ris_compress; one JSON record.

Device-resident inputs (k_i * B for seeded scalars, from zc_ed_mul_base: subgroup points in non-trivial coordinates), HIP events
on the launch stream.  Per size both paths are warmed up, then timed one after the other in every one of `--reps` rounds
(alternated in this process); a sample is `inner` back-to-back calls between two events, `inner` chosen per path so that a
sample lasts about 20 ms.  The composition's kernels are entry points this change does not touch.
Checked in the same run: the two paths give the same bytes on every row, and the first `--oracle-rows` rows are the CPU
oracle's ris_compress(ed_double(P)).
Reported per path: median, min, max in ms per call, rows/s.  `expected_factor` is what multiplication counts alone suggest
(about 274 against about 40 plus a share of an inversion, and the issue's rough 8 x); it is recorded beside the measured one, not
asserted.  Acceptance: the composition takes more than 1.03 x the new call's time (the box-to-box spread of multiplier-bound
kernels is +- 3 %).
Usage: python tools/bench_ris_double_compress.py [--sizes 20,22] [--reps 10] [--warmup 3] [--out profiles/r13_ris_double_compress.json]"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dusk_zerocaf_amd as z  # noqa: E402
from tests.vectors import rand_scalars_np  # noqa: E402

EXPECTED_FACTOR = 8.0
SPREAD = 1.03


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.dtype == np.uint8 else a.view(np.int64)).cuda()


def sample_ms(f, inner, st):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(inner):
        f()
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def run_group(paths, n, reps, warmup, st):
    inner = {}
    for name, f in paths.items():
        for _ in range(warmup):
            f()
        torch.cuda.synchronize()
        one = sample_ms(f, 1, st)
        inner[name] = max(1, min(50, math.ceil(20.0 / max(one, 1e-3))))
    times = {name: [] for name in paths}
    for _ in range(reps):
        for name, f in paths.items():
            times[name].append(sample_ms(f, inner[name], st))
    out = {}
    for name, v in times.items():
        med = float(np.median(v))
        out[name] = {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "calls_per_sample": inner[name],
                     "M_rows_per_s": round(n / med / 1e3, 1)}
    return out


def one_size(eng, oracle, lg, reps, warmup, oracle_rows, st):
    n = 1 << lg
    p = eng.ed_mul_base(dev(rand_scalars_np(n, 13000 + lg, 249)))
    new = eng.ris_double_and_compress(p)
    old = eng.ris_compress(eng.ed_double(p))
    m = min(n, oracle_rows)
    head = p[:m].cpu().numpy().view(np.uint64)
    want = oracle.ris_compress(oracle.mt(oracle.ed_double, head))
    rec = {"rows": n, "reps": reps,
           "every_row_identical_to_the_composition": bool((new == old).all()),
           "oracle_rows": m, "oracle_parity": bool(np.array_equal(new[:m].cpu().numpy(), want))}
    del new, old
    t = run_group({"ris_double_and_compress": lambda: eng.ris_double_and_compress(p),
                   "ed_double_then_ris_compress": lambda: eng.ris_compress(eng.ed_double(p))}, n, reps, warmup, st)
    rec.update(t)
    rec["composition_over_new"] = round(t["ed_double_then_ris_compress"]["median_ms"] / t["ris_double_and_compress"]["median_ms"], 3)
    rec["expected_factor"] = EXPECTED_FACTOR
    rec["beats_the_composition_by_more_than_the_spread"] = rec["composition_over_new"] > SPREAD
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20,22")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--oracle-rows", type=int, default=1 << 16)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from oracle import zc_ref as oracle
    oracle.build()
    oracle.lib()
    eng = z.Engine([0])
    st = torch.cuda.current_stream()
    eng.set_stream(st.cuda_stream)
    rec = {"lib": eng.lib.zc_version().decode(), "device": torch.cuda.get_device_name(0), "sizes": []}
    for lg in (int(x) for x in args.sizes.split(",")):
        r = one_size(eng, oracle, lg, args.reps, args.warmup, args.oracle_rows, st)
        print(json.dumps(r), file=sys.stderr, flush=True)
        rec["sizes"].append(r)
        torch.cuda.empty_cache()
    eng.close()
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    ok = all(s["every_row_identical_to_the_composition"] and s["oracle_parity"] and s["beats_the_composition_by_more_than_the_spread"] for s in rec["sizes"])
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
