#!/usr/bin/env python3
"""zc_ris_lincomb against the best composition the library offered before it, one JSON record.

For every shape (terms t, base term or not, rows n), once with every array on the device and once from host (numpy) arrays:
every path warmed up, then `--reps` rounds in which the paths are timed one after the other (alternated in this process,
host clock around a device synchronisation):
  * fused:        one Engine.ris_lincomb call;
  * composition:  t ris_decompress calls on per-term encodings copied contiguous beforehand, their points gathered row-major,
                  ed_lincomb, (base term) ed_mul_base + ed_add, ris_compress;
  * composition_one_decode: the same with ONE ris_decompress over the n * t encodings (its output is row-major as it is).
Every output row of the paths is compared byte for byte (the inputs are valid encodings: every row decodes).
Reported per path: median, min, max in ms; fused rows/s; the field multiplications per row of the fused call by part (one
decode per term, 1827 + 567 t for the tables and the window loop, 33 mixed additions for the base term, one encode).
Device-resident gate: the fused median is not above the composition's median by more than the composition's own
(max - min) spread; the same comparison against the one-decode variant is recorded beside it.  Host arrays: the ratio is recorded beside the bytes per row the two paths move over PCIe, counted from
the record sizes; it is not gated.
Usage: python tools/bench_ris_lincomb.py [--shapes 1:1:20,2:0:20,7:1:18] [--reps 10] [--warmup 2] [--out profiles/r11_ris_lincomb.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dusk_zerocaf_amd as z  # noqa: E402
from tests.vectors import rand_scalars_np  # noqa: E402
from tools.bench_msm_fixed import sync_ms  # noqa: E402


def muls_per_row(t, base):
    """Field multiplications per row of the fused call, by part (decode and encode are one fixed exponentiation each)."""
    return {"decodes": t, "tables_and_window_loop": 1827 + 567 * t, "base_term_mixed_additions": 33 if base else 0, "encodes": 1}


def pcie_bytes(t, base):
    """Bytes per row over PCIe when every array is host memory, from the record sizes."""
    fused = 32 * t + 40 * t + (40 if base else 0) + 32 + 1
    comp = (32 + 160 + 1) * t + (160 * t + 40 * t + 160) + ((40 + 160) + (320 + 160) if base else 0) + (160 + 32)
    return {"fused": fused, "composition": comp, "predicted_ratio": round(comp / fused, 2)}


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.dtype == np.uint8 else a.view(np.int64)).cuda()


def inputs(eng, t, base, n, seed):
    """Valid encodings r_ij * B (device), 252-bit scalars; per-term contiguous copies of the encodings."""
    E = eng.ris_compress(eng.ed_mul_base(dev(rand_scalars_np(n * t, seed, 249)))).view(n, t, 32)
    K = dev(rand_scalars_np(n * t, seed + 1, 252).reshape(n, t, 5))
    KB = dev(rand_scalars_np(n, seed + 2, 252)) if base else None
    return E, K, KB, [E[:, j].contiguous() for j in range(t)]


def compose(eng, E, K, KB, cols, one_decode):
    host = isinstance(K, np.ndarray)
    n, t = K.shape[:2]
    if one_decode:
        D = eng.ris_decompress(E.reshape(n * t, 32))[0].reshape(n, t, 20)
    else:
        pts = [eng.ris_decompress(c)[0] for c in cols]
        D = np.stack(pts, axis=1) if host else torch.stack(pts, dim=1)
    acc = eng.ed_lincomb(D, K)
    if KB is not None:
        acc = eng.ed_add(acc, eng.ed_mul_base(KB))
    return eng.ris_compress(acc)


def timed(f, host):
    if not host:
        return sync_ms(f)
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def one_residency(eng, E, K, KB, cols, reps, warmup, host):
    paths = {"fused": lambda: eng.ris_lincomb(E, K, KB),
             "composition": lambda: compose(eng, E, K, KB, cols, False),
             "composition_one_decode": lambda: compose(eng, E, K, KB, cols, True)}
    for _ in range(warmup):
        for f in paths.values():
            f()
    times = {name: [] for name in paths}
    same = True
    for _ in range(reps):
        outs = {}
        for name, f in paths.items():
            ms, outs[name] = timed(f, host)
            times[name].append(ms)
        got, ok = outs["fused"]
        for name in ("composition", "composition_one_decode"):
            same = same and bool((got == outs[name]).all()) and bool((ok == 1).all())
    rec = {name: stats(v) for name, v in times.items()}
    rec["every_row_identical"] = same
    best = min(("composition", "composition_one_decode"), key=lambda name: rec[name]["median_ms"])
    rec["best_composition"] = best
    rec["fused_over_best_composition"] = round(rec["fused"]["median_ms"] / rec[best]["median_ms"], 4)
    return rec


def one_shape(eng, t, base, lg, reps, warmup, seed):
    n = 1 << lg
    E, K, KB, cols = inputs(eng, t, base, n, seed)
    rec = {"terms": t, "base_term": bool(base), "rows": n, "reps": reps, "muls_per_row_fused": muls_per_row(t, base)}
    d = one_residency(eng, E, K, KB, cols, reps, warmup, False)
    def gate(name):
        b = d[name]
        return {"against": name, "allowed_ms": round(b["median_ms"] + b["max_ms"] - b["min_ms"], 4),
                "met": bool(d["fused"]["median_ms"] <= b["median_ms"] + (b["max_ms"] - b["min_ms"]) and d["every_row_identical"])}
    # the gate: against the composition a caller had (per-term decodes); the one-decode variant is reported the same way
    d["gate"] = dict(gate("composition"), rule="fused median <= composition median + its (max - min)")
    d["against_one_decode"] = gate("composition_one_decode")
    d["rows_per_s"] = round(n / (d["fused"]["median_ms"] / 1e3))
    rec["device_resident"] = d
    hE, hK, hKB = E.cpu().numpy(), K.cpu().numpy().view(np.uint64), None if KB is None else KB.cpu().numpy().view(np.uint64)
    h = one_residency(eng, hE, hK, hKB, [np.ascontiguousarray(hE[:, j]) for j in range(t)], reps, warmup, True)
    h["pcie_bytes_per_row"] = pcie_bytes(t, base)
    h["measured_ratio_best_composition_over_fused"] = round(h[h["best_composition"]]["median_ms"] / h["fused"]["median_ms"], 3)
    rec["host_arrays"] = h
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1:1:20,2:0:20,7:1:18")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split(":")) for s in a.shapes.split(",")]
    eng = z.Engine()
    rec = {"lib": eng.lib.zc_version().decode(), "device": torch.cuda.get_device_name(0), "shapes": []}
    for i, (t, base, lg) in enumerate(shapes):
        r = one_shape(eng, t, bool(base), lg, a.reps, a.warmup, 5000 + 10 * i)
        print(json.dumps(r), file=sys.stderr, flush=True)
        rec["shapes"].append(r)
    eng.close()
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    ok = all(r["device_resident"]["gate"]["met"] and r["host_arrays"]["every_row_identical"] for r in rec["shapes"])
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
