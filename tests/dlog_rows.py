"""Generators, rows and the truth for the tests of the bounded discrete logs (zc_dlog_create, zc_ed_dlog, zc_ris_dlog: CPU
emulation, planted defects and GPU tier).

Every expected answer is PLANTED: a found row is P = m * G from the oracle's ed_scalar_mul (for the wire form its ris_compress on
top) with m < bound.  A not-found row is not found by construction: m >= bound, (L - 1) * G, or m * G + T with T a point of E[8]
(tests/point_classes.py) -- and by the order argument of include/zerocaf_hip_dlog.h: the order of G_eff is a multiple of L, so no
second m below 2^38 gives the same point.  Nothing is taken from the code under test.

The m list is built from the constants of dusk_zerocaf_amd/csrc/zc_dlog_plan.h, read from its text: with C = DLOG_CHUNK,
S = DLOG_STEPS_PER_LAUNCH and T = 2^t the edges of a table (0, 1, T - 1, T, T + 1), of a chunk ((C - 1) T + T - 1, C T, C T + 1),
of a launch (S T - 1, S T, S T + 1) and of the bound, which is no multiple of T: bound - 1 is found, bound and bound + 1 -- in the
same, last giant step -- are not.  Tables of at most 64 records are asked for every baby step.  Every row comes a second time
scaled by a random Z."""
import ctypes as C
import os
import re

import numpy as np

from oracle import pymodel as pm
from tests import gens_rows as GR
from tests import point_classes as PC
from tests import vectors as V
from tests.emul_build import CSRC

SEED = V.SEED + 0xD106
COSET4 = 1
GENERATORS = ("B", "multiple", "mixed")
WIRE_GENERATORS = ("B", "multiple")                 # their multiples lie in <B>: ris_compress takes them
EMPTY = (1 << 64) - 1
MIX = 0x9E3779B97F4A7C15

_cache = {}


def plan_constants():
    """DLOG_CHUNK, DLOG_STEPS_PER_LAUNCH, ... as zc_dlog_plan.h states them."""
    if "plan" not in _cache:
        text = open(os.path.join(CSRC, "zc_dlog_plan.h")).read()
        get = lambda name: int(re.search(r"constexpr \w+ %s = (\d+)u?;" % name, text).group(1))
        _cache["plan"] = dict(chunk=int(re.search(r"^#define ZC_DLOG_CHUNK (\d+)$", text, flags=re.M).group(1)), steps_per_launch=get("DLOG_STEPS_PER_LAUNCH"), min_bits=get("DLOG_MIN_BITS"), max_bits=get("DLOG_MAX_BITS"),
                              max_steps=get("DLOG_MAX_STEPS"), block=get("DLOG_BLOCK"), setup_stride=get("DLOG_SETUP_STRIDE"), setup_w=get("DLOG_SETUP_W"))
    return _cache["plan"]


def rows_of(*rows):
    return np.ascontiguousarray(np.array(rows, dtype=np.uint64).reshape(-1, 20))


def generator(oracle, name):
    """(20,), read-only.  B: the basepoint; multiple: r * B in other coordinates (Z != 1, T holds garbage: the library reads X, Y
    and Z); mixed: B + T8, order 8 L."""
    key = ("G", name)
    if key not in _cache:
        B = GR.basepoint()
        if name == "B":
            G = B[0].copy()
        elif name == "multiple":
            G = PC.scale(oracle, PC.subgroup(oracle, 1, SEED + 1), SEED + 2)[0]
            assert G[10:15].tolist() != pm.limbs(1)
            G[15:] = np.array(GR.GARBAGE_T, dtype=np.uint64)
        else:
            G = oracle.ed_add(B, PC.torsion(oracle)[1:2])[0]
            assert PC.order_in_e8(oracle, PC.times_L(oracle, rows_of(G))) == 8
        assert oracle.ed_is_valid(rows_of(G))[0] == 1
        G.setflags(write=False)
        _cache[key] = G
    return _cache[key]


def multiples(oracle, G, ms):
    """m * G for the integers ms, by the oracle's Mul<Scalar>: (len(ms), 20)."""
    P = np.ascontiguousarray(np.tile(GR.with_true_t(oracle, rows_of(G)), (len(ms), 1)))
    k = np.array([pm.limbs(int(m)) for m in ms], dtype=np.uint64)
    return oracle.mt(oracle.ed_scalar_mul, P, k)


def bound_for(t):
    """Past the second launch's first giant step and no multiple of 2^t: the last giant step holds bound - 1, bound and bound + 1."""
    c = plan_constants()
    T = 1 << t
    return c["steps_per_launch"] * T + 3 * T + 5


def found_values(t, bound=None):
    c, T = plan_constants(), 1 << t
    Ck, S = c["chunk"], c["steps_per_launch"]
    bound = bound or bound_for(t)
    ms = [0, 1, T - 1, T, T + 1, (Ck - 1) * T + T - 1, Ck * T, Ck * T + 1, S * T - 1, S * T, S * T + 1, bound - 1]
    ms += list(range(T)) if T <= 64 else [int(j) for j in np.random.default_rng(SEED + t).integers(0, T, 24)]
    out = []
    for m in ms:
        if m not in out and m < bound:
            out.append(m)
    return out


def missed_values(t, bound=None):
    bound = bound or bound_for(t)
    return [bound, bound + 1, bound + 5 * (1 << t), 2 * bound + 3, pm.L - 1]


def ed_rows(oracle, name, t, coset4, bound=None):
    """dict(points (n, 20), m (n,), found (n,), what [n]): found rows, missed rows, torsion rows, then all of them scaled."""
    key = ("ed", name, t, bool(coset4), bound)
    if key not in _cache:
        G = generator(oracle, name)
        b = bound or bound_for(t)
        T, S = 1 << t, plan_constants()["steps_per_launch"]
        hit, miss = found_values(t, b), missed_values(t, b)
        pts = [multiples(oracle, G, hit + miss)]
        m = hit + [0] * len(miss)
        found = [1] * len(hit) + [0] * len(miss)
        what = ["m=%d" % v for v in hit] + ["m=%d (not below the bound)" % v for v in miss]
        tors = PC.torsion(oracle)
        base = [1, T + 1, S * T + 1]
        under = multiples(oracle, G, base)
        for j in range(1, 8):
            pts.append(oracle.ed_add(under, np.ascontiguousarray(np.tile(tors[j], (len(base), 1)))))
            in_e4 = j % 2 == 0
            m += [v if coset4 and in_e4 else 0 for v in base]
            found += [1 if coset4 and in_e4 else 0] * len(base)
            what += ["m=%d + %d T8" % (v, j) for v in base]
        pts = np.concatenate(pts)
        scaled = PC.scale(oracle, pts, SEED + 7 + t)
        assert not np.array_equal(scaled, pts) and oracle.mt(oracle.ed_eq, scaled, np.ascontiguousarray(pts)).all()
        out = dict(points=np.ascontiguousarray(np.concatenate([pts, scaled])), m=np.array(m + m, dtype=np.uint64), found=np.array(found + found, dtype=np.uint8),
                   what=what + [w + " scaled" for w in what], bound=b)
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def bad_encodings(oracle, n):
    """(n, 32) byte rows the oracle's ris_decompress refuses: all ones, a negative s, then seeded random bytes."""
    if "bad" not in _cache:
        rng = np.random.default_rng(SEED + 11)
        cand = np.concatenate([np.full((1, 32), 0xFF, dtype=np.uint8), np.frombuffer(int(pm.P - 1).to_bytes(32, "little"), dtype=np.uint8).reshape(1, 32),
                               rng.integers(0, 256, size=(64, 32), dtype=np.uint8)])
        _, ok = oracle.ris_decompress(np.ascontiguousarray(cand))
        _cache["bad"] = np.ascontiguousarray(cand[ok == 0])
        assert len(_cache["bad"]) >= 8
    return _cache["bad"][:n]


def wire_rows(oracle, name, t, bound=None):
    """dict(enc (n, 32), m, found, ok): encodings of found and missed multiples, the identity (32 zero bytes, m = 0) and rows that
    do not decode.  For tables with ZC_DLOG_COSET4."""
    key = ("wire", name, t, bound)
    if key not in _cache:
        G = generator(oracle, name)
        b = bound or bound_for(t)
        hit, miss = found_values(t, b), missed_values(t, b)
        enc = oracle.mt(oracle.ris_compress, multiples(oracle, G, hit + miss))
        assert not enc[0].any()                                                          # m = 0: the identity
        bad = bad_encodings(oracle, 6)
        out = dict(enc=np.ascontiguousarray(np.concatenate([enc, np.zeros((1, 32), dtype=np.uint8), bad])),
                   m=np.array(hit + [0] * (len(miss) + 1 + len(bad)), dtype=np.uint64),
                   found=np.array([1] * len(hit) + [0] * len(miss) + [1] + [0] * len(bad), dtype=np.uint8),
                   ok=np.array([1] * (len(hit) + len(miss) + 1) + [0] * len(bad), dtype=np.uint8), bound=b)
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def hostile_points(oracle):
    """(3, 20): off the curve, Z = 0 by value (X = 0, so that the projective equation holds), all-ones limbs."""
    off = np.array(GR.basepoint()[0])
    off[5] ^= np.uint64(1)
    z0 = np.array([0] * 5 + pm.limbs(5) + [0] * 5 + [0] * 5, dtype=np.uint64)
    ones = np.full(20, (1 << 64) - 1, dtype=np.uint64)
    return rows_of(off, z0, ones)


# ------------------------------------------------------------------ the record and the slot array, restated
def record_of(oracle, points):
    """(n, 4) words: canonical affine y with the parity of canonical x in bit 255, from the oracle's ed_to_affine."""
    xy, ok = oracle.ed_to_affine(np.ascontiguousarray(points, dtype=np.uint64))
    assert ok.all()
    out = np.zeros((len(xy), 4), dtype=np.uint64)
    for i, r in enumerate(xy.tolist()):
        v = pm.from_limbs(r[5:]) | ((pm.from_limbs(r[:5]) & 1) << 255)
        out[i] = [(v >> (64 * k)) & EMPTY for k in range(4)]
    return out


def effective_generator(oracle, G, coset4):
    G = GR.with_true_t(oracle, rows_of(G))
    return oracle.ed_double(oracle.ed_double(G)) if coset4 else G


def table_records(oracle, name, t, coset4):
    """(2^t, 4): the records of j * G_eff."""
    key = ("records", name, t, bool(coset4))
    if key not in _cache:
        _cache[key] = record_of(oracle, multiples(oracle, effective_generator(oracle, generator(oracle, name), coset4)[0], range(1 << t)))
    return _cache[key]


def home(w0, t):
    return ((int(w0) * MIX) & EMPTY) >> (63 - t)


def tag(w0):
    return (int(w0) * MIX) & 0xFFFFFFFF


def slots_of(records, t):
    """The slot array of zc_dlog_plan.h, restated: records filed in j order, linear probing from the top t + 1 bits of w0 * MIX,
    a slot = tag << 32 | j.  Returns (slots, displacement per record)."""
    slots = [EMPTY] * (2 << t)
    moved = []
    for j, rec in enumerate(records.tolist()):
        s = home(rec[0], t)
        d = 0
        while slots[s] != EMPTY:
            s = (s + 1) & ((2 << t) - 1)
            d += 1
        slots[s] = (tag(rec[0]) << 32) | j
        moved.append(d)
    return np.array(slots, dtype=np.uint64), moved


# ------------------------------------------------------------------ the host-emulation library (tests/emul/dlog_emul.cpp)
def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


class Table:
    def __init__(self, t, flags, setup, records, slots):
        self.t, self.flags, self.setup, self.records, self.slots = t, flags, setup, records, slots


class Emul:
    """One build of tests/emul/dlog_emul.cpp.  Outputs are framed: nothing outside rows 0 .. n-1 may be written."""

    def __init__(self, lib):
        self.lib = lib
        lib.emul_dlog_setup_words.restype = C.c_size_t
        lib.emul_dlog_steps_per_launch.restype = C.c_ulonglong
        lib.emul_dlog_slots.restype = C.c_long
        lib.emul_dlog_setup.restype = C.c_uint

    def constants(self):
        return dict(chunk=self.lib.emul_dlog_chunk(), steps_per_launch=self.lib.emul_dlog_steps_per_launch())

    def create(self, point, t, flags=0):
        """(verdict, Table or None): 0 built, 1 not a point of the curve, 2 generator in E[8], 3 a record could not be filed."""
        point = np.ascontiguousarray(point, dtype=np.uint64).reshape(20)
        setup = np.zeros(self.lib.emul_dlog_setup_words(), dtype=np.uint32)
        verdict = self.lib.emul_dlog_setup(_p(point), C.c_uint(t), C.c_uint(flags), _p(setup))
        if verdict:
            return verdict, None
        buf = np.full(4 * (1 << t) + 8, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        records = buf[4:-4]
        self.lib.emul_dlog_records(_p(setup), C.c_uint(t), _p(records))
        assert (buf[:4] == 0xA5A5A5A5A5A5A5A5).all() and (buf[-4:] == 0xA5A5A5A5A5A5A5A5).all()
        slots = np.zeros(2 << t, dtype=np.uint64)
        if self.lib.emul_dlog_slots(_p(records), C.c_uint(t), _p(slots)) != -1:
            return 3, None
        return 0, Table(t, flags, setup, records, slots)

    def record(self, point):
        out = np.zeros(4, dtype=np.uint64)
        self.lib.emul_dlog_record(_p(np.ascontiguousarray(point, dtype=np.uint64)), _p(out))
        return out

    def search(self, table, rows, bound, wire=False, cuts=None, want_ok=True):
        """(m, found, ok)."""
        rows = np.ascontiguousarray(rows, dtype=np.uint8 if wire else np.uint64)
        before, n = rows.copy(), len(rows)
        m = np.full(n + 2, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        found, ok = np.full(n + 2, 0xA5, dtype=np.uint8), np.full(n + 2, 0xA5, dtype=np.uint8)
        args = [C.c_int(int(wire)), _p(rows), C.c_size_t(n), _p(table.setup), _p(table.records), _p(table.slots), C.c_uint(table.t), C.c_uint(table.flags), C.c_uint64(bound)]
        outs = [_p(m[1:]), _p(found[1:]), _p(ok[1:]) if want_ok else None]
        if cuts is None:
            self.lib.emul_dlog(*args, *outs)
        else:
            cuts = np.array(cuts, dtype=np.uint64)
            self.lib.emul_dlog_cut(*args, _p(cuts), C.c_size_t(len(cuts)), *outs)
        assert np.array_equal(rows, before)
        for a, fill in ((m, 0xA5A5A5A5A5A5A5A5), (found, 0xA5), (ok, 0xA5)):
            assert a[0] == fill and a[-1] == fill
        if not want_ok:
            assert (ok == 0xA5).all()
        return m[1:-1].copy(), found[1:-1].copy(), ok[1:-1].copy()


EMUL_BITS = (4, 6)


def failures(lib, oracle):
    """The checks of the emulation tier on one build, as labels of those that failed: "record" (a point's record against the
    oracle's affine values), per generator, table size and flag "table" (records and slot array against their restatement), "ed"
    (zc_ed_dlog against the planted truth), "cut" (the same search cut at arbitrary giant steps); per generator of <B> "wire"
    (zc_ris_dlog); "refusals" (what is no point of the curve, generators in E[8])."""
    em, failed = Emul(lib), []
    c = plan_constants()
    pts = np.concatenate([PC.classes(oracle, 6, SEED + 20)[k] for k in ("subgroup", "order_8L", "scaled")])
    if not np.array_equal(np.stack([em.record(p) for p in pts]), record_of(oracle, pts)):
        failed.append("record")
    for name in GENERATORS:
        for t in EMUL_BITS:
            for coset4 in (0, COSET4):
                label = "[%s t=%d coset4=%d]" % (name, t, coset4)
                verdict, table = em.create(generator(oracle, name), t, coset4)
                want = table_records(oracle, name, t, coset4)
                if verdict or not np.array_equal(table.records.reshape(-1, 4), want) or not np.array_equal(table.slots, slots_of(want, t)[0]):
                    failed.append("table " + label)
                    continue
                R = ed_rows(oracle, name, t, coset4)
                m, found, ok = em.search(table, R["points"], R["bound"])
                if not (np.array_equal(m, R["m"]) and np.array_equal(found, R["found"]) and ok.all()):
                    failed.append("ed " + label)
                S, Ck = c["steps_per_launch"], c["chunk"]
                cuts = [0, Ck, 3 * Ck, S - Ck, S, S + 4]                                 # S + 4 giant steps hold every m below the bound
                m, found, ok = em.search(table, R["points"], R["bound"], cuts=cuts, want_ok=False)
                if not (np.array_equal(m, R["m"]) and np.array_equal(found, R["found"])):
                    failed.append("cut " + label)
                if coset4 and name in WIRE_GENERATORS:
                    Wr = wire_rows(oracle, name, t)
                    m, found, ok = em.search(table, Wr["enc"], Wr["bound"], wire=True)
                    if not (np.array_equal(m, Wr["m"]) and np.array_equal(found, Wr["found"]) and np.array_equal(ok, Wr["ok"])):
                        failed.append("wire " + label)
    bad = [em.create(p, 4, f)[0] for p in hostile_points(oracle)[:2] for f in (0, COSET4)]
    tors = PC.torsion(oracle)
    small = [em.create(tors[j], 4, 0)[0] for j in range(8)] + [em.create(oracle.ed_add(GR.basepoint(), tors[2:3])[0], 4, COSET4)[0]]
    hostile = hostile_points(oracle)
    _, table = em.create(generator(oracle, "B"), 4, 0)
    mixed = np.concatenate([multiples(oracle, generator(oracle, "B"), [3]), hostile, multiples(oracle, generator(oracle, "B"), [17])])
    m, found, ok = em.search(table, mixed, 64)
    if bad != [1] * 4 or small != [2] * 8 + [0] or m.tolist() != [3, 0, 0, 0, 17] or found.tolist() != [1, 0, 0, 0, 1] or ok.tolist() != [1, 0, 0, 0, 1]:
        failed.append("refusals")
    return failed
