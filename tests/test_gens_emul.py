"""CPU tier: the device functions behind the generator sets (zc_gens.hip.h: gens_normalise, gens_row_sum; zc_curve.hip.h:
comb_table_column and the basepoint comb's recoding and additions), built for the host by tests/emul/gens_emul.cpp in the plain
and the bounds-asserting (-DZC_CHECK_BOUNDS) build.  Table build and both row forms are compared with the oracle's composition
(tests/gens_rows.py): the Edwards form as a group element with its compressed bytes, the wire form byte for byte; the list [B]
with the emulated zc_ed_mul_base / zc_ris_mul_base_compress; the basepoint's table with the words it had before its builder
was generalised.  The sanitizer run is a stand-alone program (tests/emul/gens_san.cpp) replaying a vector file as a child
process: nothing sanitized is loaded here."""
import ctypes as C
import hashlib
import json
import os
import struct

import numpy as np
import pytest

from tests import emul_build as EB
from tests import gens_rows as GR
from tests.emul_build import HERE

N =GR.POOL + 37                                     # rows repeat from POOL on


@pytest.fixture(scope="module", params=["plain", "checked"])
def emul(request):
    so = EB.library("gens_emul.cpp", checked=request.param == "checked")
    if so is None:
        pytest.skip("ROCm headers not present")
    return GR.Emul(C.CDLL(so))


@pytest.fixture(scope="module")
def built(emul, oracle):
    """count -> tables, each built once per library."""
    out = {}
    for count in GR.COUNTS:
        bad, out[count] = emul.build(GR.generators(oracle, count))
        assert bad == -1, count
    return out


def test_the_rows_are_what_the_issue_asks_for(oracle):
    pool, clean = GR.scalar_pool()
    edges = [GR.pm.limbs(v) for v in GR.KV.recoding_scalars()]
    assert pool[:len(edges)].tolist() == edges and (pool > GR.M52).any() and (clean <= GR.M52).all()
    values = [GR.KV.value(r) for r in clean]
    stops = [GR.PC.effective_scalar(v) != v for v in values]
    assert sum(stops) >= 6 and sum(v >= 1 << 256 and not s for v, s in zip(values, stops)) >= 6      # at or above 2^256, with and without early stop
    for count in GR.COUNTS:
        K = GR.scalars(count)
        assert K.shape == (GR.POOL, count, 5) and len({r.tobytes() for r in K}) == GR.POOL <= 330
        for j in range(count):
            assert {r.tobytes() for r in K[:, j]} == {r.tobytes() for r in pool}                      # every scalar in every term position
        assert np.array_equal(GR.scalars(count, N)[GR.POOL:], K[:N - GR.POOL])
    G2, G3, G8 = (GR.with_true_t(oracle, GR.generators(oracle, c)) for c in (2, 3, 8))
    assert oracle.ed_eq(oracle.ed_add(G2[:1], G2[1:]), GR.PC.ident_rows(1))[0] == 1 and np.array_equal(G3[0], G3[1])
    assert GR.PC.is_identity(oracle, G8[1:2])[0] and GR.generators(oracle, 1)[0, 10:15].tolist() != GR.pm.limbs(1)


@pytest.mark.parametrize("count", GR.COUNTS)
def test_ed_form_is_the_references_sum(emul, built, oracle, count):
    K = GR.scalars(count, N)
    pts, enc = GR.want(oracle, count, N)
    got = emul.ed(built[count], K)
    GR.R.assert_same_points(oracle, got, pts)
    assert (got <= GR.M52).all()
    assert np.array_equal(oracle.mt(oracle.ris_compress, got), enc)
    # the limbs are the row's own, whatever stands beside it
    for i in (0, 5, 63, 64, GR.POOL - 1):
        assert np.array_equal(emul.ed(built[count], K[i:i + 1]), got[i:i + 1])


@pytest.mark.parametrize("count", GR.COUNTS)
def test_wire_form_gives_the_oracles_bytes(emul, built, oracle, count):
    K = GR.scalars(count, N)
    got = emul.wire(built[count], K)
    assert np.array_equal(got, GR.want(oracle, count, N)[1])
    assert np.array_equal(got, oracle.mt(oracle.ris_compress, emul.ed(built[count], K)))
    for i in (0, 64, N - 1):
        assert np.array_equal(emul.wire(built[count], K[i:i + 1]), got[i:i + 1])


def test_identity_sums_are_the_identity_and_32_zero_bytes(emul, built, oracle):
    """k G - k G (count 2: G_1 = -G_0 with equal scalars), all scalars zero, and the identity as a generator."""
    pool, _ = GR.scalar_pool()
    same = np.ascontiguousarray(np.stack([pool, pool], axis=1))
    assert GR.PC.is_identity(oracle, emul.ed(built[2], same)).all() and not emul.wire(built[2], same).any()
    for count in GR.COUNTS:
        zero = np.zeros((70, count, 5), dtype=np.uint64)
        assert GR.PC.is_identity(oracle, emul.ed(built[count], zero)).all() and not emul.wire(built[count], zero).any()
    only = np.zeros((len(pool), 8, 5), dtype=np.uint64)
    only[:, 1] = pool                                                                   # generator 1 of the list of 8 is the identity
    assert GR.PC.is_identity(oracle, emul.ed(built[8], only)).all() and not emul.wire(built[8], only).any()


def test_the_list_of_the_basepoint_agrees_with_the_basepoint_calls(emul, oracle):
    bad, t = emul.build(GR.basepoint())
    assert bad == -1
    base = emul.base_table()
    assert np.array_equal(t, base)                                                      # B's limbs are the constants: the same table
    K = GR.scalars(1, N)
    k = np.ascontiguousarray(K[:, 0])
    assert oracle.mt(oracle.ed_eq, emul.ed(t, K), emul.ed_base(base, k)).all()
    assert np.array_equal(emul.wire(t, K), emul.wire_base(base, k))
    wp, wb = GR.want_base(oracle, N)
    assert np.array_equal(emul.wire(t, K), wb) and oracle.mt(oracle.ed_eq, emul.ed(t, K), np.ascontiguousarray(wp)).all()


def test_the_basepoint_table_kept_its_words(emul):
    """base_table_column goes through the generalised builder; zc_ed_mul_base's limbs are pinned, so its table must be the old one."""
    with open(os.path.join(HERE, "golden", "base_table_sha256.json")) as f:
        gold = json.load(f)
    t = emul.base_table()
    assert t.size == gold["words"] and hashlib.sha256(t.astype("<u4").tobytes()).hexdigest() == gold["sha256"]


def test_create_refuses_what_is_no_curve_point_and_ignores_t(emul, built, oracle):
    for name, pts, first in GR.refused_lists(oracle):
        assert emul.build(pts)[0] == first, name
    for count in GR.COUNTS:                                                             # every list holds records whose T is garbage
        G = GR.generators(oracle, count)
        bad, t = emul.build(GR.with_true_t(oracle, G))
        assert bad == -1 and np.array_equal(t, built[count]) and not np.array_equal(G, GR.with_true_t(oracle, G))
    # a generator given in other coordinates builds the same table: records are normalised to Z = 1
    G = GR.generators(oracle, 2)
    scaled = GR.PC.scale(oracle, G, GR.SEED + 9)
    assert not np.array_equal(scaled, G) and np.array_equal(emul.build(scaled)[1], built[2])


def test_the_whole_tier_passes_as_the_mutant_test_runs_it(emul, oracle):
    assert GR.failures(emul.lib, oracle) == []


def test_stand_alone_program_under_asan_and_ubsan(tmp_path, oracle):
    """tests/emul/gens_san.cpp with -fsanitize=address,undefined -fno-sanitize-recover=all: tables in heap blocks of exactly
    33 * 128 * 128 * count bytes, every scalar of the pool in the first and in the last term position; its exit status is the
    verdict."""
    exe = EB.sanitizer_program("gens_san.cpp", tmp_path)
    parts, rows = [], 0
    for count in (1, 3):
        G, K, enc = GR.generators(oracle, count), GR.scalars(count), GR.want(oracle, count)[1]
        parts.append(struct.pack("<2Q", count, len(K)) + GR.with_true_t(oracle, G).tobytes() + K.tobytes() + np.ascontiguousarray(enc).tobytes())
        rows += len(K)
    blob = b"".join(parts) + struct.pack("<Q", 0)
    EB.assert_clean(EB.run_vectors(exe, blob, tmp_path, "vectors.bin"), "2 records, %d rows match" % rows)
    bad = bytearray(blob)
    bad[-9] ^= 1                                                                        # the last byte of the last expected encoding
    EB.assert_caught(EB.run_vectors(exe, bad, tmp_path, "wrong.bin"), "record 1: row %d: word 3" % (GR.POOL - 1))
