#!/usr/bin/env python3
"""CPU model of the strict scalar-mul schedule of k_ed_scalar_mul_pw (zc_curve.hip.h: sm_lane): how many generic steps
(9 multiplications) and wave-uniform doubling steps a 64-lane tile performs, and what that is worth in multiplier-class
instructions against the unified-step schedule (every step generic).  No GPU, no library: the numbers are an
instruction-count model, not a measurement.

Inputs as bench.py's headline: seeded 252-bit scalars, sorted by cost (bit length - 1 + popcount, most expensive first, as
k_sm_cost_* do) and cut into tiles of 64.  A lane does double_and_add's operations in order; a doubling may run ahead of
up to `depth` pending additions (their addends wait in a per-lane stash).  Per wave step:
  * generic step: every active lane does one thing -- its oldest pending addition if it has one, else its doubling;
  * doubling step (wave-uniform): every active lane doubles, its pending addition (if any) joining the stash.  Possible
    iff no lane is BLOCKED (pending addition for its current bit and the stash full) and every active lane is below its
    top bit.  (--sit-out: also when lanes at their top bit would have to sit the step out: no better when alternating, one
    step per tile worse with --greedy);
  * policy "alternate" (the kernel's, default): a doubling step only right after a generic step; --greedy: whenever possible.
    At depth 1 no lane is blocked after a generic step, and two doubling steps in a row are possible only when no lane of
    the 64 added anything in between: the two policies differ on sparse scalars only.
depth 0 is "doubling steps only when no lane wants an addition"; --no-d-steps is the unified schedule itself.
Depth 1 is what the kernel implements (one 144-byte slot per lane is what fits LDS at three workgroups per CU).

Usage: python tools/sm_schedule_model.py [--n 1048576] [--seed 0x5EED0003] [--tiles 128] [--depths 0,1,2,4] [--sit-out] [--greedy]
"""
import argparse

import numpy as np

WAVE = 64
MUL, SQR = 135 + 25, 99 + 25            # v_mad_u64_u32 + (9 v_mul_lo_u32, 16 64-bit shifts) per multiplication / squaring
GENERIC = 9 * MUL                        # 1440
DOUBLINGS = {"3S+5M": 3 * SQR + 5 * MUL,     # 1172: ptm_double_valid (needs the validity gate)
             "4S+5M": 4 * SQR + 5 * MUL}     # 1296: squarings only where the generic formula's operands are equal


def effective(v):
    """The scalar double_and_add multiplies by (zc_curve.hip.h: scalar_effective): the loop stops at the smallest T with
    (v >> T) mod 2^256 == 0 and returns (v mod 2^T) * P."""
    v &= (1 << 260) - 1
    t = 0
    while (v >> t) % (1 << 256):
        t += 1
    return v % (1 << t)


def cost(v):
    v = effective(v)
    return v.bit_length() - 1 + bin(v).count("1") if v else 0


def tile_steps(scalars, depth=1, d_steps=True, sit_out=False, greedy=False):
    """(generic steps, doubling steps, stashed addends) of one tile; `scalars`: up to 64 Python integers."""
    vals = [effective(int(v)) for v in scalars]
    lanes = len(vals)
    bits = np.zeros((lanes, 261), dtype=bool)
    for j, v in enumerate(vals):
        bits[j] = np.unpackbits(np.frombuffer(v.to_bytes(33, "little"), dtype=np.uint8), bitorder="little")[:261]
    nbits = np.array([v.bit_length() for v in vals])
    ar = np.arange(lanes)
    pos = np.zeros(lanes, dtype=int)
    stash = np.zeros(lanes, dtype=int)
    taken = np.zeros(lanes, dtype=bool)
    active = nbits > 0
    g = d = stashed = 0
    last_was_d = True                                    # the kernel starts every tile with a generic step
    while active.any():
        pending = bits[ar, pos] & ~taken & active
        needs = active & (pos < nbits - 1)
        blocked = needs & pending & (stash >= depth)
        if d_steps and (greedy or not last_was_d) and not blocked.any() and needs.any() and (sit_out or not (active & ~needs).any()):
            put = needs & pending
            stash[put] += 1
            stashed += int(put.sum())
            pos[needs] += 1
            taken[needs] = False
            d += 1
            last_was_d = True
        else:
            from_stash = active & (stash > 0)
            stash[from_stash] -= 1
            add = active & ~from_stash & pending
            taken[add] = True
            dbl = active & ~from_stash & ~add
            pos[dbl] += 1
            taken[dbl] = False
            g += 1
            last_was_d = False
            active &= (pos < nbits - 1) | ~taken | (stash > 0)
    return g, d, stashed


def bench_scalars(n, seed, bits=252):
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 1 << 52, size=(n, 5), dtype=np.uint64)
    k[:, 4] = rng.integers(0, 1 << (bits - 208), size=n, dtype=np.uint64)
    return k


def to_ints(k):
    return [sum(int(x) << (52 * j) for j, x in enumerate(row)) for row in k]


def sorted_tiles(k, tiles):
    """`tiles` evenly spaced 64-lane tiles of the cost-sorted batch (most expensive first), as lists of integers."""
    pop = np.zeros(len(k), dtype=np.int64)
    blen = np.zeros(len(k), dtype=np.int64)
    for j in range(5):
        x = k[:, j].copy()
        nz = x != 0
        top = np.zeros(len(k), dtype=np.int64)
        while x.any():
            pop += (x & np.uint64(1)).astype(np.int64)
            top += (x != 0)
            x >>= np.uint64(1)
        blen = np.where(nz, 52 * j + top, blen)
    c = np.where(blen > 0, blen - 1 + pop, 0)
    order = np.argsort(-c, kind="stable")
    ntiles = len(k) // WAVE
    step = max(1, ntiles // tiles)
    return [to_ints(k[order[t * WAVE:(t + 1) * WAVE]]) for t in range(0, ntiles, step)], float(c.mean())


def model(tiles, depth, d_steps=True, sit_out=False, greedy=False):
    """Mean steps per tile and the instruction ratios against the unified schedule for the two doubling bodies."""
    G = D = S = base = 0
    for vals in tiles:
        g, d, s = tile_steps(vals, depth, d_steps, sit_out, greedy)
        G, D, S = G + g, D + d, S + s
        base += max(cost(v) for v in vals)              # unified schedule: the dearest lane's cost
    m = len(tiles)
    return {"generic": G / m, "doubling": D / m, "unified": base / m, "stashed_per_lane": S / m / WAVE,
            "ratio": {name: (G * GENERIC + D * c) / (base * GENERIC) for name, c in DOUBLINGS.items()}}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=lambda s: int(s, 0), default=1 << 20)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x5EED0003)
    ap.add_argument("--tiles", type=int, default=128, help="evenly spaced tiles of the sorted batch to simulate")
    ap.add_argument("--depths", default="0,1,2,4")
    ap.add_argument("--no-d-steps", action="store_true")
    ap.add_argument("--sit-out", action="store_true")
    ap.add_argument("--greedy", action="store_true")
    a = ap.parse_args()
    tiles, mean_cost = sorted_tiles(bench_scalars(a.n, a.seed), a.tiles)
    print("n = %d, seed = %#x, %d tiles simulated, mean cost %.1f" % (a.n, a.seed, len(tiles), mean_cost))
    print("%-6s %10s %10s %10s %12s   %s" % ("depth", "generic", "doubling", "unified", "stash/lane", "  ".join("%8s" % n for n in DOUBLINGS)))
    for depth in [int(x) for x in a.depths.split(",")]:
        r = model(tiles, depth, not a.no_d_steps, a.sit_out, a.greedy)
        print("%-6d %10.1f %10.1f %10.1f %12.1f   %s" % (depth, r["generic"], r["doubling"], r["unified"], r["stashed_per_lane"],
                                                       "  ".join("%8.4f" % r["ratio"][n] for n in DOUBLINGS)))


if __name__ == "__main__":
    main()
