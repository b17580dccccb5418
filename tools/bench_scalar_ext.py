#!/usr/bin/env python3
"""The scalar operations for protocols against what the library offered before them, one JSON record.

Device-resident inputs (canonical scalars below 2^249, random bytes), HIP events on the launch stream.  Per size and group the
paths are warmed up, then timed one after the other in every one of `--reps` rounds (alternated in this process); a sample
is `inner` back-to-back calls between two events, `inner` chosen per path so that a sample lasts about 20 ms.  Groups:
  * invert:   zc_sc_invert  |  zc_sc_pow(a, L - 2)  |  zc_fe_invert on the same words (same schedule, longer modulus)
  * muladd:   zc_sc_muladd(a, b, c)  |  zc_sc_mul then zc_sc_add
  * reduce:   zc_sc_from_bytes_wide (104 B/row)  |  zc_sc_from_bytes_mod_order (72 B/row)  |  zc_sc_from_bytes (73 B/row)
The baselines are entry points this change does not touch.  Outputs of the new calls are compared with the baselines' on
every row (invert with pow, muladd with mul + add; the reduction of values below L with from_bytes).
Reported per path: median, min, max in ms per call, rows/s, algorithmic GB/s from the bytes per row.
Usage: python tools/bench_scalar_ext.py [--sizes 20,24] [--reps 10] [--warmup 3] [--out profiles/r12_scalar_ext.json]"""
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
from oracle import pymodel as pm  # noqa: E402
from tests.vectors import rand_scalars_np  # noqa: E402

BYTES = {"sc_invert": 81, "sc_pow_L_minus_2": 120, "fe_invert": 81, "sc_muladd": 160, "sc_mul_then_sc_add": 240,
         "sc_from_bytes_wide": 104, "sc_from_bytes_mod_order": 72, "sc_from_bytes": 73}


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
                     "M_rows_per_s": round(n / med / 1e3, 1), "bytes_per_row": BYTES[name], "alg_GBps": round(BYTES[name] * n / med / 1e6, 1)}
    return out


def one_size(eng, lg, reps, warmup, st):
    n = 1 << lg
    a, b, c = (dev(rand_scalars_np(n, 7000 + lg + j, 249)) for j in range(3))
    e = dev(np.tile(np.array(pm.limbs(pm.L - 2), dtype=np.uint64), (n, 1)))
    rng = np.random.default_rng(7100 + lg)
    wide = dev(rng.integers(0, 256, size=(n, 64), dtype=np.uint8))
    narrow = eng.sc_to_bytes(a)                                                   # values below L: all three 32-byte paths accept them
    rec = {"rows": n, "reps": reps}
    same = {"invert_equals_pow": bool((eng.sc_invert(a)[0] == eng.sc_pow(a, e)).all()),
            "muladd_equals_mul_then_add": bool((eng.sc_muladd(a, b, c) == eng.sc_add(eng.sc_mul(a, b), c)).all()),
            "mod_order_equals_from_bytes_below_L": bool((eng.sc_from_bytes_mod_order(narrow) == eng.sc_from_bytes(narrow)[0]).all()
                                                        and (eng.sc_from_bytes_mod_order(narrow) == a).all())}
    rec["every_row_identical"] = same
    inv = run_group({"sc_invert": lambda: eng.sc_invert(a), "sc_pow_L_minus_2": lambda: eng.sc_pow(a, e), "fe_invert": lambda: eng.fe_invert(a)},
                    n, reps, warmup, st)
    inv["sc_invert_over_fe_invert"] = round(inv["sc_invert"]["median_ms"] / inv["fe_invert"]["median_ms"], 4)
    inv["sc_pow_over_sc_invert"] = round(inv["sc_pow_L_minus_2"]["median_ms"] / inv["sc_invert"]["median_ms"], 2)
    rec["invert"] = inv
    mad = run_group({"sc_muladd": lambda: eng.sc_muladd(a, b, c), "sc_mul_then_sc_add": lambda: eng.sc_add(eng.sc_mul(a, b), c)}, n, reps, warmup, st)
    mad["composition_over_muladd"] = round(mad["sc_mul_then_sc_add"]["median_ms"] / mad["sc_muladd"]["median_ms"], 4)
    rec["muladd"] = mad
    rec["reduce"] = run_group({"sc_from_bytes_wide": lambda: eng.sc_from_bytes_wide(wide), "sc_from_bytes_mod_order": lambda: eng.sc_from_bytes_mod_order(narrow),
                               "sc_from_bytes": lambda: eng.sc_from_bytes(narrow)}, n, reps, warmup, st)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20,24")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    eng = z.Engine([0])
    st = torch.cuda.current_stream()
    eng.set_stream(st.cuda_stream)
    rec = {"lib": eng.lib.zc_version().decode(), "device": torch.cuda.get_device_name(0), "sizes": []}
    for lg in (int(x) for x in args.sizes.split(",")):
        r = one_size(eng, lg, args.reps, args.warmup, st)
        print(json.dumps(r), file=sys.stderr, flush=True)
        rec["sizes"].append(r)
        torch.cuda.empty_cache()
    eng.close()
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    return 0 if all(all(s["every_row_identical"].values()) for s in rec["sizes"]) else 1


if __name__ == "__main__":
    sys.exit(main())
