#!/usr/bin/env python3
"""Generator sets: zc_ed_mul_gens and zc_ris_mul_gens_compress against the calls a caller composes without them, one JSON record.

Device-resident inputs, HIP events on the context's stream.  Per pair both sides are warmed up, then timed one after the other
in every one of `--reps` rounds (alternated in this process, at least seven); a sample is `inner` back-to-back calls between two
events, `inner` chosen per side so that a sample lasts about 20 ms.  Every pair carries a `parity` flag from a comparison of
whole outputs in the same run (encodings for the Edwards form: the calls return other representatives) and the run-to-run
spread of either side.
  * base:   one generator, the curve basepoint:  zc_ed_mul_gens | zc_ed_mul_base  and  zc_ris_mul_gens_compress |
            zc_ris_mul_base_compress -- the same arithmetic from another table pointer: the ratio must lie within the spread
  * ed (a): zc_ed_mul_gens(k)            |  zc_ed_lincomb(G tiled into every row, k)
  * ed (b): zc_ed_mul_gens(k)            |  count x zc_ed_mul_gens over one-generator sets + (count - 1) x zc_ed_add
  * wire:   zc_ris_mul_gens_compress(k)  |  zc_ris_lincomb(encodings of G tiled into every row, k, no base term)
`count_ratio` beside every measured ratio is the ratio of field multiplications per row: 231 per term (33 mixed
additions of 7), 250 for ris_compress, against 1827 + 567 t for zc_ed_lincomb and 265 per decoded term.  Also recorded: the
time of zc_gens_create for 1 and 8 generators (host clock around the synchronous call), and the Edwards form per row and term
at 1, 2, 4 and 8 generators on the same rows (the tables of 8 generators, 4.3 MB, outgrow the 4 MiB L2 of an XCD).
The scalars are seeded 248-bit values, the generators seeded multiples of the basepoint.
Usage: python tools/bench_gens.py [--base 16,20,22] [--cases 20:2,20:4,18:8] [--per-term 18] [--reps 7] [--warmup 2] [--out profiles/r20_gens.json]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TERM, COMPRESS, DECODE = 231, 250, 265          # field multiplications: one comb term, ris_compress, ris_decompress
LINCOMB = lambda t: 1827 + 567 * t


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
    """paths: {name: callable}; the sides alternate in every round."""
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
    pair["ratio_gens_over_replaced"] = round(pair[new]["median_ms"] / pair[old]["median_ms"], 4)
    pair["count_ratio"] = round(count_ratio, 4) if count_ratio else None
    pair["spread"] = max(pair[new]["spread"], pair[old]["spread"])
    pair["below_by_more_than_the_spread"] = pair["ratio_gens_over_replaced"] < 1.0 - pair["spread"]
    pair["within_the_spread"] = abs(pair["ratio_gens_over_replaced"] - 1.0) <= pair["spread"]
    return pair


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", default="16,20,22", help="lg(rows) of the one-generator comparison with the basepoint calls")
    ap.add_argument("--cases", default="20:2,20:4,18:8", help="lg(rows):count, comma-separated")
    ap.add_argument("--per-term", type=int, default=18, help="lg(rows) of the per-term series at 1, 2, 4 and 8 generators")
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
    rng = np.random.default_rng(2000)
    rand_sc = lambda n: np.array([pm.limbs(int.from_bytes(rng.bytes(40), "little") % pm.L) for _ in range(n)], dtype=np.uint64)
    rand_dev = lambda shape: torch.from_numpy(np.concatenate([rng.integers(0, 1 << 52, size=shape + (4,), dtype=np.uint64),
                                                              rng.integers(0, 1 << 40, size=shape + (1,), dtype=np.uint64)], axis=-1).view(np.int64)).cuda()
    G = eng.ed_mul_base(rand_sc(8))                                             # (8, 20) host: the generators
    B = np.array([sum(pm.pt_limbs(pm.BASEPOINT), [])], dtype=np.uint64)
    rec = {"lib": eng.lib.zc_version().decode(), "device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
           "multiplications": {"term": TERM, "ris_compress": COMPRESS, "ris_decompress": DECODE, "zc_ed_lincomb": "1827 + 567 t"},
           "base": [], "cases": [], "create": [], "per_term": []}
    ok = True

    # ---- zc_gens_create
    for count in (1, 8):
        ms = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            g = eng.generators(G[:count])
            ms.append((time.perf_counter() - t0) * 1e3)
            g.close()
        rec["create"].append({"count": count, "median_ms": round(float(np.median(ms[1:])), 3), "min_ms": round(min(ms[1:]), 3), "max_ms": round(max(ms[1:]), 3),
                              "first_ms": round(ms[0], 3), "table_bytes": count * 33 * 128 * 128})

    # ---- one generator, the basepoint, against the basepoint calls
    gb = eng.generators(B)
    for lg in [int(x) for x in args.base.split(",") if x]:
        n = 1 << lg
        K = rand_dev((n, 1))
        k = K.reshape(n, 5)
        entry = {"lg_rows": lg, "rows": n}
        new, old = (lambda: eng.ed_mul_gens(gb, K)), (lambda: eng.ed_mul_base(k))
        a, b = new(), old()
        parity = bool(eng.ed_eq(a, b).all())
        del a, b
        pair = run_pair({"zc_ed_mul_gens": new, "zc_ed_mul_base": old}, args.reps, args.warmup, st)
        entry["ed"] = finish(pair, "zc_ed_mul_gens", "zc_ed_mul_base", parity, 1.0)
        ok = ok and parity
        new, old = (lambda: eng.ris_mul_gens_compress(gb, K)), (lambda: eng.ris_mul_base_compress(k))
        parity = bool((new() == old()).all())
        pair = run_pair({"zc_ris_mul_gens_compress": new, "zc_ris_mul_base_compress": old}, args.reps, args.warmup, st)
        entry["wire"] = finish(pair, "zc_ris_mul_gens_compress", "zc_ris_mul_base_compress", parity, 1.0)
        ok = ok and parity
        entry["rows_per_s_ed"] = round(n / entry["ed"]["zc_ed_mul_gens"]["median_ms"] * 1e3)
        entry["rows_per_s_wire"] = round(n / entry["wire"]["zc_ris_mul_gens_compress"]["median_ms"] * 1e3)
        print("basepoint, 2^%d rows: ed %.4f, wire %.4f of the basepoint calls (spread %.4f / %.4f, parity %s)" % (
            lg, entry["ed"]["ratio_gens_over_replaced"], entry["wire"]["ratio_gens_over_replaced"], entry["ed"]["spread"], entry["wire"]["spread"],
            entry["ed"]["parity"] and parity), file=sys.stderr, flush=True)
        rec["base"].append(entry)
        del K, k
        torch.cuda.empty_cache()
    gb.close()

    # ---- 2, 4, 8 generators against the compositions
    for case in [c for c in args.cases.split(",") if c]:
        lg, t = [int(x) for x in case.split(":")]
        n = 1 << lg
        g = eng.generators(G[:t])
        singles = [eng.generators(G[j:j + 1]) for j in range(t)]
        K = rand_dev((n, t))
        cols = [K[:, j:j + 1].contiguous() for j in range(t)]
        Gd = torch.from_numpy(G[:t].view(np.int64)).cuda()
        P = Gd.reshape(1, t, 20).expand(n, t, 20).contiguous()
        E = eng.ris_compress(Gd).reshape(1, t, 32).expand(n, t, 32).contiguous()
        entry = {"lg_rows": lg, "rows": n, "count": t, "tiled_point_bytes_per_row": 160 * t}
        new, tiled = (lambda: eng.ed_mul_gens(g, K)), (lambda: eng.ed_lincomb(P, K))

        def compose():
            acc = eng.ed_mul_gens(singles[0], cols[0])
            for j in range(1, t):
                acc = eng.ed_add(acc, eng.ed_mul_gens(singles[j], cols[j]))
            return acc
        a, b, c = new(), tiled(), compose()
        ea = eng.ed_compress(a)[0]
        parity = bool((ea == eng.ed_compress(b)[0]).all()) and bool((ea == eng.ed_compress(c)[0]).all()) and bool(eng.ed_eq(a, b).all())
        del a, b, c, ea
        pair = run_pair({"zc_ed_mul_gens": new, "zc_ed_lincomb_tiled_G": tiled}, args.reps, args.warmup, st)
        entry["ed_vs_lincomb"] = finish(pair, "zc_ed_mul_gens", "zc_ed_lincomb_tiled_G", parity, TERM * t / LINCOMB(t))
        pair = run_pair({"zc_ed_mul_gens": new, "mul_gens_per_generator_and_add": compose}, args.reps, args.warmup, st)
        entry["ed_vs_composition"] = finish(pair, "zc_ed_mul_gens", "mul_gens_per_generator_and_add", parity, TERM * t / (TERM * t + 9 * (t - 1)))
        ok = ok and parity
        wnew, wtiled = (lambda: eng.ris_mul_gens_compress(g, K)), (lambda: eng.ris_lincomb(E, K))
        a, (b, bok) = wnew(), wtiled()
        parity = bool((a == b).all()) and bool(bok.all())
        del a, b, bok
        pair = run_pair({"zc_ris_mul_gens_compress": wnew, "zc_ris_lincomb_tiled_G": wtiled}, args.reps, args.warmup, st)
        entry["wire_vs_ris_lincomb"] = finish(pair, "zc_ris_mul_gens_compress", "zc_ris_lincomb_tiled_G", parity,
                                              (TERM * t + COMPRESS) / (LINCOMB(t) + DECODE * t + COMPRESS))
        ok = ok and parity
        entry["rows_per_s_ed"] = round(n / entry["ed_vs_lincomb"]["zc_ed_mul_gens"]["median_ms"] * 1e3)
        entry["rows_per_s_wire"] = round(n / entry["wire_vs_ris_lincomb"]["zc_ris_mul_gens_compress"]["median_ms"] * 1e3)
        print("2^%d rows, %d generators: ed/lincomb %.4f, ed/composition %.4f, wire %.4f (parity %s)" % (
            lg, t, entry["ed_vs_lincomb"]["ratio_gens_over_replaced"], entry["ed_vs_composition"]["ratio_gens_over_replaced"],
            entry["wire_vs_ris_lincomb"]["ratio_gens_over_replaced"], parity and entry["ed_vs_lincomb"]["parity"]), file=sys.stderr, flush=True)
        rec["cases"].append(entry)
        for s in singles + [g]:
            s.close()
        del P, E, K, cols
        torch.cuda.empty_cache()

    # ---- the Edwards form per row and term on the same rows
    n = 1 << args.per_term
    series = {}
    sets = {t: eng.generators(G[:t]) for t in (1, 2, 4, 8)}
    Ks = {t: rand_dev((n, t)) for t in sets}
    timed = run_pair({"count_%d" % t: (lambda t=t: eng.ed_mul_gens(sets[t], Ks[t])) for t in sets}, args.reps, args.warmup, st)
    for t in sets:
        r = timed["count_%d" % t]
        series[t] = r["median_ms"] * 1e6 / (n * t)
        rec["per_term"].append({"lg_rows": args.per_term, "count": t, "median_ms": r["median_ms"], "spread": r["spread"], "ns_per_row_and_term": round(series[t], 4),
                                "table_bytes": t * 33 * 128 * 128})
        sets[t].close()
    rec["per_term_8_over_4"] = round(series[8] / series[4], 4)
    print("ns per row and term at 1 / 2 / 4 / 8 generators: %s" % " / ".join("%.3f" % series[t] for t in (1, 2, 4, 8)), file=sys.stderr, flush=True)
    eng.close()
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
