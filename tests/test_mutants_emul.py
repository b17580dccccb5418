"""CPU tier: every planted defect of tests/mutants.py must be caught by the kill-vector family it names.

Per entry the headers (dusk_zerocaf_amd/csrc/*.h) and the emulation sources (tests/emul/*.cpp) are copied into a temporary
directory, the one replacement is applied to the copy, the one emulation library the entry's family needs is built from it
with g++ (as the other emulation fixtures build theirs, no sanitizer), loaded with ctypes and the family run in-process: at
least one comparison must fail.  The unmutated copy must pass every family, every `old` text must occur exactly once in its
header, and the canary (fe_carry stopping at limb 7) must be killed.  Nothing is written inside the repository tree; the
builds run on a thread pool of at most 16."""
import ctypes as C
import os

import pytest

from tests import emul_build as EB
from tests import kill_vectors as KV
from tests import mutants as M
from tests.emul_build import HERE

HEADERS = {M.ARITH: "zc_arith.hip.h", M.CURVE: "zc_curve.hip.h"}
BY_NAME = {m["name"]: m for m in M.MUTANTS}


def kind(m):
    if "equivalent" in m:
        return "equivalent"
    if "rounds" in m and 30 * m["rounds"] >= M.S_MAX[m["family"][-1]]:          # longest_inversions_p / _l
        return "not reached"
    return "killed"


def families_of(m):
    return m["survives"] if "equivalent" in m else (m["family"],)


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """{entry name or None (the unmutated copy): {library: path}}: per entry the libraries its families load."""
    return EB.mutant_builds(tmp_path_factory, M.MUTANTS, KV.LIBS, headers=HEADERS, needs=lambda m: sorted({KV.FAMILIES[f].lib for f in families_of(m)}), workers=16)


def failures(built, name, family):
    lib = C.CDLL(built[name][KV.FAMILIES[family].lib])
    return KV.run(family, KV.EmulBackend(lib))


def test_catalogue_is_sound():
    EB.catalogue_is_sound(M.MUTANTS, headers=HEADERS)
    assert len(M.MUTANTS) >= 40
    for m in M.MUTANTS:
        assert all(f in KV.FAMILIES for f in families_of(m)), m["name"]
        assert ("equivalent" in m) != ("family" in m) and ("equivalent" not in m or len(m["equivalent"]) > 80), m["name"]
    kinds = [kind(m) for m in M.MUTANTS]
    assert kinds.count("equivalent") <= 0.15 * len(kinds), kinds.count("equivalent")
    # every family is the named killer of at least one entry: take a family away and that entry fails
    assert {m["family"] for m, k in zip(M.MUTANTS, kinds) if k == "killed"} == set(KV.FAMILIES)
    assert sum(1 for m in M.MUTANTS if m.get("canary")) == 1
    # the rounds rule: S_MAX is the file's, the largest schedule that is too short for it is in the catalogue and must be killed
    worst = KV.divsteps_worst()
    assert M.S_MAX == {"p": worst["s_max_p"], "l": worst["s_max_l"]}
    for key in ("p", "l"):
        assert worst["s_max_" + key] == max(e["steps"] for e in worst[key]) and len(worst[key]) == 64
        need = -(-M.S_MAX[key] // 30) - 1
        assert any(m.get("rounds") == need and m["family"] == "longest_inversions_" + key and kind(m) == "killed" for m in M.MUTANTS), (key, need)


def test_recorded_step_counts_are_the_models():
    """The counts in tests/golden/divsteps_worst.json, recomputed with the generator's own step model."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_divsteps_worst", os.path.join(HERE, "golden", "gen_divsteps_worst.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    worst = KV.divsteps_worst()
    for key, mod in (("p", KV.P), ("l", KV.L)):
        assert all(gen.steps_needed(int(e["a"], 16), mod) == e["steps"] and 0 < int(e["a"], 16) < mod for e in worst[key])
        assert M.S_MAX[key] > {"p": 524, "l": 518}[key] and M.S_MAX[key] <= 600         # beats plain sampling; within the schedule


def test_second_subtraction_is_out_of_reach():
    """The bound behind the `equivalent` entries of mod_invert_chunk, on the exact register value of the Montgomery multiplier,
    (T + ((T N') mod R) N) / R with R = 2^261: the running product of a lane stays below 2N for chunks of 2, 7 and 64 rows of
    the largest five-word patterns (and of seeded patterns next to 2^260), so does every a_j^-1 and every quotient."""
    import random
    R = 1 << 261
    rng = random.Random(KV.SEED + 0x2A)
    for N in (KV.P, KV.L):
        NP = (-pow(N, -1, R)) % R

        def mont(a, b):
            T = a * b
            v, rem = divmod(T + (T * NP % R) * N, R)
            assert rem == 0
            return v
        big = [(1 << 260) - 1 - d for d in range(4)] + [(1 << 260) - 1 - rng.getrandbits(k) for k in (8, 64, 130, 200, 250, 259)]
        for c in (2, 7, 64):
            for trial in range(12):
                xs = [big[trial % len(big)]] * c if trial < len(big) else [rng.choice(big) for _ in range(c)]
                acc, pre = R % N, []
                for x in xs:
                    pre.append(acc)
                    acc = mont(acc, x)
                    assert acc < 2 * N
                inv = pow(acc % N, -1, N)
                for x, q in zip(reversed(xs), reversed(pre)):
                    res = mont(inv, q)
                    assert res < 2 * N and res % N == pow(x, -1, N)
                    assert mont((1 << 260) - 1, mont(res, R * R % N)) < 2 * N          # the division form, largest numerator
                    inv = mont(inv, x)
                    assert inv < 2 * N


@pytest.mark.parametrize("family", sorted(KV.FAMILIES))
def test_unmutated_copy_passes(built, family):
    assert failures(built, None, family) == []


def test_canary_is_killed(built):
    m = [m for m in M.MUTANTS if m.get("canary")][0]
    assert failures(built, m["name"], m["family"]) != []


def killing(built, name, family):
    """[(case, outputs, indices of the outputs that differ)] of the comparisons the changed build fails in one family."""
    backend = KV.EmulBackend(C.CDLL(built[name][KV.FAMILIES[family].lib]))
    out = []
    for case in KV.FAMILIES[family].cases():
        got = backend.call(case)
        bad = case.mismatches(got) if got is not None else []
        if bad:
            out.append((case, got, bad))
    return out


ONE_PASS_ONLY = ("plain_fold_", "from_limbs52_shl_low_limb", "to_limbs52_shr_offset")       # lines only the one-pass product runs


def test_killing_rows_are_carried(built):
    """What kills a defect here must be what the GPU tier can carry into every launch form (tests/test_gpu_kill_vector_forms.py
    tiles the rowwise cases).  Per killed entry, from the emulation's failed comparisons and the rows that differ:
      * if a failed comparison is one the C ABI reaches (kill_vectors.EngineBackend.reach: the operation exists there and a
        differing output is one it returns), at least one such case is rowwise;
      * entries without any are listed -- found by that rule, not kept by hand: their killers are digit strings, effective
        scalars, step counts, the interleaved multiplier or a Jacobi schedule of three rounds, which exist in the emulation only;
      * a defect killed through `mulmod`: the emulation chooses the product form per row, the device per wave, so every
        killing row must sit, in the one-pass packing, in a wave whose rows all reach as far above 2^TOPBIT as it does (the
        ballot then decides as the row alone would) -- eligible killing rows in all-eligible waves; the defects in lines only
        the one-pass product runs must have such rows."""
    problems, emulation_only = [], []
    for m in M.MUTANTS:
        if kind(m) != "killed":
            continue
        failed = killing(built, m["name"], m["family"])
        assert failed, m["name"]
        reached = [(case, got, bad) for case, got, bad in failed if set(bad) & set(KV.EngineBackend.reach(case))]
        if not reached:
            emulation_only.append("%s (%s)" % (m["name"], ", ".join(sorted({case.label() for case, _, _ in failed}))))
            continue
        if not any(case.rowwise for case, _, _ in reached):
            problems.append("%s: no rowwise case among %s" % (m["name"], [case.label() for case, _, _ in reached]))
        eligible_killers = 0
        for case, got, bad in reached:
            if case.op != "mulmod":
                continue
            for output, which in ((0, "mul"), (1, "sq")):
                rows = case.bad_rows(got, output)
                lv = KV.mulmod_levels(case, which)
                order = KV.pack_order(lv, "one-pass")
                as_alone = set(order[KV.wave_levels(lv[order]) == lv[order]].tolist())
                eligible_killers += sum(1 for r in rows if lv[r] == 0)
                if not set(rows) <= as_alone:
                    problems.append("%s: %s rows %s of %s sit in no wave that decides as they do" % (m["name"], which, sorted(set(rows) - as_alone), case.label()))
        if m["name"].startswith(ONE_PASS_ONLY) and not eligible_killers:
            problems.append("%s: no killing row is eligible for the one-pass product" % m["name"])
    print("killed in the emulation only (no failed comparison the C ABI reaches):")
    for line in emulation_only:
        print("    " + line)
    assert problems == []


@pytest.mark.parametrize("name", [m["name"] for m in M.MUTANTS])
def test_planted_defect(built, name):
    m = BY_NAME[name]
    k = kind(m)
    for family in families_of(m):
        failed = failures(built, name, family)
        if k == "killed":
            assert failed != [], "%s survived family %s" % (name, family)
        else:                                  # equivalent, or a schedule no recorded input exceeds: the claim itself is checked
            assert failed == [], (name, k, family, failed)
