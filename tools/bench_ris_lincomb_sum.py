#!/usr/bin/env python3
"""zc_ris_lincomb_sum against (a) per-row verification with zc_ris_lincomb on the same rows and (b) the hand composition of
public calls it replaces: zc_ris_decompress, one zc_sc_muladd per term and one for the base term, a host-side sum of the n
base terms, zc_msm over n terms + 1 pairs, zc_ris_compress on one point.  One JSON record.

Device-resident inputs (encodings of k_i * B from zc_ris_mul_base_compress, canonical scalars, 128-bit weights), HIP events on
the launch stream.  Per shape the three paths are warmed up, then timed one after the other in every one of `--reps` rounds
(alternated in this process); a sample is `inner` back-to-back calls between two events.  (a) answers a different question
-- every row's own result -- and is there as the cost of verifying row by row; (b) computes the same 32 bytes.  (b)'s sum of
the base terms crosses to the host and back, as a caller has to do it today: that copy is part of its time.
Checked in the same run: the call and (b) give the same bytes; the call's bytes are the CPU oracle's on the first
`--oracle-rows` rows (a call of their own); (a)'s rows are the oracle's on the first 4096 rows.
No ratio is fixed in advance: the measured times and their spread are recorded.
Usage: python tools/bench_ris_lincomb_sum.py [--shapes 2x20,7x18] [--reps 10] [--warmup 2] [--out profiles/r14_ris_lincomb_sum.json]"""
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
from tests import ris_lincomb_rows as RR  # noqa: E402
from tests import ris_sum_rows as RS  # noqa: E402
from tests.vectors import rand_scalars_np  # noqa: E402


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.dtype == np.uint8 else a.view(np.int64)).cuda()


def host(t):
    a = t.cpu().numpy()
    return a if a.dtype == np.uint8 else a.view(np.uint64)


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
        inner[name] = max(1, min(20, math.ceil(20.0 / max(one, 1e-3))))
    times = {name: [] for name in paths}
    for _ in range(reps):
        for name, f in paths.items():
            times[name].append(sample_ms(f, inner[name], st))
    out = {}
    for name, v in times.items():
        med = float(np.median(v))
        out[name] = {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "spread": round(max(v) / min(v), 4),
                     "calls_per_sample": inner[name], "M_rows_per_s": round(n / med / 1e3, 1)}
    return out


def composition(eng, E, K, KB, Z, basepoint):
    """The hand composition on device tensors: (32 bytes, ok)."""
    n, t = E.shape[:2]
    D, okj = eng.ris_decompress(E.reshape(n * t, 32))
    ok = (okj.reshape(n, t) != 0).all(dim=1)
    zero = torch.zeros_like(KB)
    W = torch.stack([eng.sc_muladd(Z, K[:, j].contiguous(), zero) for j in range(t)], dim=1)
    W = W * ok.reshape(n, 1, 1)                                                  # an undecodable term removes the whole row
    tb = host(eng.sc_muladd(Z, KB, zero) * ok.reshape(n, 1))
    # there is no device reduction among the public calls: column sums of the 52-bit limbs in two 32-bit halves (no overflow
    # below 2^32 rows), put together as a Python integer
    lo, hi = (tb & np.uint64(0xFFFFFFFF)).sum(axis=0), (tb >> np.uint64(32)).sum(axis=0)
    b = sum((int(l) + (int(h) << 32)) << (52 * i) for i, (l, h) in enumerate(zip(lo, hi))) % pm.L
    P = torch.cat([D, basepoint])
    S = torch.cat([W.reshape(n * t, 5), dev(np.array([pm.limbs(b)], dtype=np.uint64))])
    return bytes(eng.ris_compress(eng.msm(P, S))[0]), ok


def one_shape(eng, oracle, t, lg, reps, warmup, oracle_rows, st):
    n = 1 << lg
    seed = 14000 + 100 * t + lg
    E = eng.ris_mul_base_compress(dev(rand_scalars_np(n * t, seed, 249))).reshape(n, t, 32)
    K = dev(RS.canonical_scalars(n * t, seed + 1)).reshape(n, t, 5)
    KB, Z = dev(RS.canonical_scalars(n, seed + 2)), dev(RS.weights128(n, seed + 3))
    basepoint = dev(RR.basepoint_rows(1))
    new, ok = eng.ris_lincomb_sum(E, K, KB, Z)
    comp, cok = composition(eng, E, K, KB, Z, basepoint)
    m = min(n, oracle_rows)
    hE, hK, hKB, hZ = (host(x[:m]) for x in (E, K, KB, Z))
    part, _ = eng.ris_lincomb_sum(E[:m].contiguous(), K[:m].contiguous(), KB[:m].contiguous(), Z[:m].contiguous())
    rows, rok = eng.ris_lincomb(E[:4096].contiguous(), K[:4096].contiguous(), KB[:4096].contiguous())
    rec = {"terms": t, "base_term": True, "rows": n, "pairs": n * t + 1, "reps": reps,
           "all_rows_accepted": bool(ok.all()) and bool(cok.all()),
           "same_bytes_as_the_composition": new == comp,
           "oracle_rows": m, "oracle_parity": part == RS.expected(oracle, hE, hK, hKB, hZ)[0],
           "per_row_oracle_parity": bool(np.array_equal(host(rows), RR.oracle_ris_lincomb(oracle, hE[:4096], hK[:4096], hKB[:4096])[0])) and bool(rok.all())}
    tms = run_group({"ris_lincomb_sum": lambda: eng.ris_lincomb_sum(E, K, KB, Z),
                     "a_per_row_ris_lincomb": lambda: eng.ris_lincomb(E, K, KB),
                     "b_hand_composition": lambda: composition(eng, E, K, KB, Z, basepoint)}, n, reps, warmup, st)
    rec.update(tms)
    rec["per_row_over_call"] = round(tms["a_per_row_ris_lincomb"]["median_ms"] / tms["ris_lincomb_sum"]["median_ms"], 3)
    rec["composition_over_call"] = round(tms["b_hand_composition"]["median_ms"] / tms["ris_lincomb_sum"]["median_ms"], 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2x20,7x18", help="terms x log2(rows), comma-separated; every shape has a base term")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--oracle-rows", type=int, default=1 << 13)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from oracle import zc_ref as oracle
    oracle.build()
    oracle.lib()
    eng = z.Engine([0])
    st = torch.cuda.current_stream()
    eng.set_stream(st.cuda_stream)
    rec = {"lib": eng.lib.zc_version().decode(), "device": torch.cuda.get_device_name(0), "shapes": []}
    for t, lg in ((int(a), int(b)) for a, b in (x.split("x") for x in args.shapes.split(","))):
        r = one_shape(eng, oracle, t, lg, args.reps, args.warmup, args.oracle_rows, st)
        print(json.dumps(r), file=sys.stderr, flush=True)
        rec["shapes"].append(r)
        torch.cuda.empty_cache()
    eng.close()
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    ok = all(s["same_bytes_as_the_composition"] and s["oracle_parity"] and s["per_row_oracle_parity"] and s["all_rows_accepted"] for s in rec["shapes"])
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
