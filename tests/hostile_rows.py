"""Hostile rows: data outside the contract, planted beside valid rows (CPU emulation tier and GPU tier).

The property under test is isolation: a row whose words are outside the contract may get any documented answer of its own, but
it must not change one byte of what any other row of the batch gets.  The harness runs a call on clean inputs (which the
caller checks against the oracle), writes patterns from the catalogue below over a row set S, runs again, and compares every
output of every row outside S byte for byte with the clean run.

Where rows share work -- Montgomery's trick shares one inversion among the rows of a lane: fe_invert_chunk,
ed_to_affine_chunk, k_msm_prepare_affine -- S is constructed from the launch geometry (hostile_set) and the construction is
asserted (check_hostile_set), so that a test cannot pass while testing nothing.

The expected answer of a hostile row itself is the answer for the VALUE its words hold, sum (w_i mod 2^52) 2^(52 i) mod p,
computed here on Python integers; a value of 0 mod p fails closed (out = 0, ok = 0) whatever its words are."""
import numpy as np

from oracle import pymodel as pm

M52 = (1 << 52) - 1
ALL_ONES = (1 << 64) - 1


def value(words):
    """What the device arithmetic reads from five u64 words: bits >= 2^52 of a word are ignored."""
    return sum((int(w) & M52) << (52 * i) for i, w in enumerate(words))


def zero_by_value(words):
    return value(words) % pm.P == 0


def narrow(words):
    """Every word below 2^52: the patterns the bounds-checked emulation build accepts."""
    return all(int(w) <= M52 for w in words)


def fe_patterns():
    """[(name, five words)]"""
    pats = [("zeros", [0] * 5)]
    pats += [("%d p" % k, pm.limbs(k * pm.P)) for k in (1, 2, 37, 255)]          # 255 p < 2^260 <= 256 p
    pats += [("p - 1", pm.limbs(pm.P - 1)), ("p + 1", pm.limbs(pm.P + 1)), ("2^252", pm.limbs(1 << 252)),
             ("all limbs 2^52 - 1", [M52] * 5), ("bit 52 of word 0", [1 << 52, 0, 0, 0, 0]), ("bit 52 of word 4", [0, 0, 0, 0, 1 << 52]),
             ("all 64 bits of every word", [ALL_ONES] * 5)]
    assert all(len(w) == 5 and all(0 <= int(x) <= ALL_ONES for x in w) for _, w in pats)
    assert [zero_by_value(w) for _, w in pats] == [True] * 5 + [False] * 4 + [True, True, False]
    return pats


def point_patterns(valid, junk_seed=0x5EED77):
    """[(name, twenty words)] around one valid point record `valid` (X | Y | Z | T)."""
    valid = [int(x) for x in valid]
    pats = [("all-zero record", [0] * 20)]
    for name, w in fe_patterns():
        pats.append(("Z = " + name, valid[:10] + [int(x) for x in w] + valid[15:]))
    import random
    rng = random.Random(junk_seed)
    junk = [pm.limbs(rng.randrange(pm.P)) for _ in range(3)]
    pats.append(("off the curve", junk[0] + junk[1] + valid[10:15] + junk[2]))
    pats.append(("every coordinate p", pm.limbs(pm.P) * 4))
    pats.append(("every word 2^52 - 1", [M52] * 20))
    pats.append(("every word all ones", [ALL_ONES] * 20))
    return pats


def undecodable(decompress):
    """[(name, 32 bytes)]: the first small integer whose little-endian bytes `decompress` (the oracle's) rejects, and 0xFF."""
    for v in range(1, 64):
        b = np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint8)
        if decompress(b.reshape(1, 32))[1][0] == 0:
            return [("undecodable %d" % v, b.copy()), ("all 0xFF", np.full(32, 0xFF, dtype=np.uint8))]
    raise AssertionError("no undecodable encoding among the small integers")


# ------------------------------------------------------------------ the answers for the value (Python integers)
def fe_invert_model(den):
    v = value(den) % pm.P
    return (pm.limbs(pow(v, pm.P - 2, pm.P)), 1) if v else ([0] * 5, 0)


def fe_div_model(num, den):
    v = value(den) % pm.P
    return (pm.limbs(value(num) * pow(v, pm.P - 2, pm.P) % pm.P), 1) if v else ([0] * 5, 0)


def ed_to_affine_model(row):
    z = value(row[10:15]) % pm.P
    if not z:
        return [0] * 10, 0
    zi = pow(z, pm.P - 2, pm.P)
    return pm.limbs(value(row[0:5]) * zi % pm.P) + pm.limbs(value(row[5:10]) * zi % pm.P), 1


# ------------------------------------------------------------------ which rows are hostile
def lane_stride(n, c, stride=None):
    """Rows i, i + stride, i + 2 stride, ... share a lane.  The field kernels launch ceil(n / c) lanes; the MSM normalisation
    rounds the lanes up to whole workgroups (pass its stride)."""
    return stride if stride is not None else -(-n // c)


def hostile_set(n, c, stride=None):
    """Sorted hostile rows for a shared-inversion call over n rows at c rows per lane: rows 0 and n - 1, and -- where a lane
    holds three rows or more -- a middle position of a second lane, a second row in the lane of row n - 1, and the last row
    of the last lane when the last chunk is ragged (that lane is then a short one).  At two rows per lane a lane cannot
    hold a middle position, nor two hostile rows beside a clean one: rows 0 (first position) and n - 1 (last position) are
    all there is.  c = 1 shares nothing."""
    st = lane_stride(n, c, stride)
    S = {0, n - 1}
    if c >= 3:
        lanes = min(st, n)
        r = list(range(1 % lanes, n, st))
        if len(r) >= 3:
            S.add(r[len(r) // 2])
        r = list(range((n - 1) % st, n, st))               # the lane of row n - 1: a second hostile row
        if len(r) >= 3:
            S.add(r[1])
        short = list(range(lanes - 1, n, st))              # the last lane is a short one whenever the last chunk is ragged
        if 2 <= len(short) < len(r):
            S.add(short[-1])
    S = sorted(S)
    check_hostile_set(S, n, c, stride)
    return S


def check_hostile_set(S, n, c, stride=None):
    """The conditions a hostile set must meet, computed from S alone."""
    S = sorted(set(int(i) for i in S))
    assert S[0] == 0 and S[-1] == n - 1, "rows 0 and n - 1 must be hostile"
    assert len(S) * 10 <= n, "more than 10 %% of the rows are hostile: %d of %d" % (len(S), n)
    st = lane_stride(n, c, stride)
    if c < 2:
        return
    lanes = min(st, n)
    counts = [len(range(g, n, st)) for g in range(lanes)]
    longest = max(counts)
    assert longest <= c
    seen = {"first": False, "middle": False, "last": False, "double": False, "short": False}
    for g in sorted({i % st for i in S}):
        pos = [i // st for i in S if i % st == g]
        cnt = counts[g]
        if len(pos) == cnt:
            continue                                       # no clean row shares this lane: it shows nothing
        seen["first"] |= 0 in pos
        seen["last"] |= cnt - 1 in pos
        seen["middle"] |= any(0 < q < cnt - 1 for q in pos)
        seen["double"] |= len(pos) >= 2
        seen["short"] |= cnt < longest
    need = ["first", "last"] if longest >= 2 else []
    if longest >= 3:
        need += ["middle", "double"]
        if any(2 <= k < longest for k in counts):
            need.append("short")                           # the ragged last chunk
    missing = [k for k in need if not seen[k]]
    assert not missing, "hostile set for (n, c) = (%d, %d) lacks %s" % (n, c, missing)


def plant(arr, S, patterns, turn):
    """Write patterns over the rows S of `arr` (in place), rotated by `turn`: over len(patterns) turns every pattern visits
    every hostile row.  Returns [(row, pattern name, words)]."""
    done = []
    for j, i in enumerate(S):
        name, w = patterns[(j + turn) % len(patterns)]
        arr[i] = np.array(w, dtype=arr.dtype)
        done.append((i, name, w))
    return done


def clean_mask(n, S):
    m = np.ones(n, dtype=bool)
    m[list(S)] = False
    return m


def assert_others_unchanged(clean, hostile, S, what=""):
    """Every output (values, ok masks, flag bytes) of every row outside S is byte-identical in the two runs."""
    if not isinstance(clean, tuple):
        clean, hostile = (clean,), (hostile,)
    assert len(clean) == len(hostile)
    for k, (a, b) in enumerate(zip(clean, hostile)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype
        keep = clean_mask(len(a), S)
        same = (a[keep].reshape(int(keep.sum()), -1) == b[keep].reshape(int(keep.sum()), -1)).all(axis=1)
        assert same.all(), "%s: output %d of clean rows %s changed (hostile rows %s)" % (what, k, np.flatnonzero(keep)[~same][:16], list(S)[:16])
