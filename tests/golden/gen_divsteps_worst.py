"""Generator of tests/golden/divsteps_worst.json: for p and for L, the 64 inputs found that need the most division steps
in the modular inversion of zc_curve.hip.h (fe_inverse_divsteps: 20 rounds of 30 steps, scheduled for the proven bound).

Only the Python model of the step rule below is used -- a transcription of sgcd_divsteps30 on full-width integers: with
zeta = -1 at the start, (f, g) = (N, a),
    g odd and zeta < 0:  (f, g, zeta) <- (g, (g - f) / 2, -zeta - 2)
    g odd:               (g, zeta)    <- ((g + f) / 2, zeta - 1)
    g even:              (g, zeta)    <- (g / 2, zeta - 1)
and the inversion is complete at the first step after which g = 0.  Random inputs need about 500 steps and never more than
~525 in 3 x 10^4 trials; the search keeps the best random starts and climbs over bit flips of the input within a fixed,
seeded budget, so a re-run writes the same file.

    python tests/golden/gen_divsteps_worst.py          (under a minute)
"""
import json
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from oracle import pymodel as pm  # noqa: E402

SEED = 0xD1F57E95
KEEP = 64
RANDOM_STARTS = 20000
CLIMB_EVALUATIONS = 150000


def steps_needed(a, n):
    """Division steps until g = 0 for (f, g) = (n, a), 0 < a < n."""
    f, g, zeta, count = n, a, -1, 0
    while g:
        if g & 1:
            if zeta < 0:
                f, g, zeta = g, (g - f) >> 1, -zeta - 2
            else:
                g, zeta = (g + f) >> 1, zeta - 1
        else:
            g, zeta = g >> 1, zeta - 1
        count += 1
    return count


def search(n, seed):
    rng = random.Random(seed)
    bits = n.bit_length()
    pool = {}
    for _ in range(RANDOM_STARTS):
        a = rng.randrange(1, n)
        pool[a] = steps_needed(a, n)
    pool = dict(sorted(pool.items(), key=lambda kv: (-kv[1], kv[0]))[:KEEP])
    floor = min(pool.values())
    for it in range(CLIMB_EVALUATIONS):
        keys = sorted(pool)
        a = keys[it % len(keys)]
        for _ in range(1 + rng.randrange(3)):
            a ^= 1 << rng.randrange(bits)
        if not 0 < a < n or a in pool:
            continue
        s = steps_needed(a, n)
        if s >= floor:
            pool[a] = s
            if len(pool) > KEEP:
                worst = min(pool.items(), key=lambda kv: (kv[1], -kv[0]))[0]
                del pool[worst]
                floor = min(pool.values())
    return sorted(pool.items(), key=lambda kv: (-kv[1], kv[0]))


def main():
    out = {"model": "half-delta division steps, zeta = -1, (f, g) = (N, a); count = first step after which g = 0",
           "seed": SEED, "random_starts": RANDOM_STARTS, "climb_evaluations": CLIMB_EVALUATIONS}
    for k, (name, n) in enumerate((("p", pm.P), ("l", pm.L))):
        found = search(n, SEED + k)
        out[name] = [{"a": "%x" % a, "steps": s} for a, s in found]
        out["s_max_" + name] = found[0][1]
        print(name, "S_max", found[0][1], "min kept", found[-1][1])
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "divsteps_worst.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
