"""CPU tier: the per-lane functions behind zc_sha512_rows, zc_sc_from_sha512 and zc_ris_from_sha512 (zc_hash.hip.h:
sha512_compress, the message reader in its word and byte forms, the two fused tails), built for the host by
tests/emul/hash_emul.cpp in the plain and the bounds-asserting (-DZC_CHECK_BOUNDS) build.  Digests are compared with hashlib,
scalars with Python integers, points with the oracle (tests/hash_rows.py); the tables with constants derived from the primes.
The sanitizer run is a stand-alone program (tests/emul/hash_san.cpp) replaying a vector file as a child process: nothing
sanitized is loaded here."""
import ctypes as C
import hashlib
import struct

import numpy as np
import pytest

from tests import emul_build as EB
from tests import hash_rows as HR
from tests import scalar_ext_rows as S
from tests import vectors as V


@pytest.fixture(scope="module", params=["plain", "checked"])
def emul(request):
    so = EB.library("hash_emul.cpp", checked=request.param == "checked")
    if so is None:
        pytest.skip("ROCm headers not present")
    return C.CDLL(so)


def sha(m):
    return hashlib.sha512(m).digest()


def check_digests(lib, parts, prefix, forms=("auto", "bytes"), offsets=(0,)):
    """Every form and offset against hashlib; returns the forms that ran at offset 0 (1: word, 0: byte)."""
    want = HR.digests(parts, prefix)
    ran = []
    for off in offsets:
        for form in forms:
            got, f = HR.emul_rows(lib, 0, parts, prefix, force_bytes=form == "bytes", offset=off)
            assert np.array_equal(got, want), (len(prefix), [p.shape[1] for p in parts], form, off)
            assert f == (1 if form == "auto" and off % 8 == 0 and HR.aligned(prefix, [p.shape[1] for p in parts]) else 0)
            if off == 0:
                ran.append(f)
    return ran


# ------------------------------------------------------------------ constants and known answers
def test_tables_are_the_roots_of_the_primes(emul):
    """80 round constants = the first 64 fractional bits of the cube roots of the first 80 primes, 8 initial values = the same
    of the square roots of the first 8: derived with integers, compared with what the header holds."""
    k, iv = HR.emul_tables(emul)
    assert HR.first_primes(80)[-1] == 409 and len(set(k)) == 80
    assert k == HR.round_constants() and iv == HR.initial_values()
    assert k[0] == 0x428a2f98d728ae22 and iv[0] == 0x6a09e667f3bcc908          # FIPS 180-4, 4.2.3 / 5.3.5: the derivation itself


def test_known_answers(emul):
    """FIPS 180-4 "abc" and the 112-byte two-block message through the rows (one part; byte form: 3 and 112 + prefix splits)
    and through the compression function alone; the empty message and one million 'a' through the compression function."""
    abc = bytes.fromhex("ddaf35a193617abacc417349ae20413112e6fa4e89a97ea20a9eeee64b55d39a2192992a274fc1a836ba3c23a3feebbd"
                        "454d4423643ce80e2a9ac94fa54ca49f")
    two = bytes.fromhex("8e959b75dae313da8cf4f72814fc143f8f7779c6eb9f7fa17299aeadb6889018501d289e4900f7e4331b99dec4b5433a"
                        "c7d329eeb6dd26545e96e55b874be909")
    assert sha(HR.FIPS_ABC) == abc and sha(HR.FIPS_TWO_BLOCKS) == two and len(HR.FIPS_TWO_BLOCKS) == 112
    for msg, want in ((HR.FIPS_ABC, abc), (HR.FIPS_TWO_BLOCKS, two)):
        row = np.frombuffer(msg, dtype=np.uint8).reshape(1, -1)
        for force in (False, True):
            assert HR.emul_rows(emul, 0, [row], force_bytes=force)[0][0].tobytes() == want
        assert HR.emul_rows(emul, 0, [row[:, 1:]], prefix=msg[:1])[0][0].tobytes() == want
        assert HR.emul_stream(emul, msg) == want
    assert HR.emul_stream(emul, b"") == sha(b"")
    assert sha(b"").hex().startswith("cf83e1357eefb8bdf1542850d66d8007d620e4050b5715dc83f4a921d36ce9ce")
    million = b"a" * 1000000
    assert HR.emul_stream(emul, million) == sha(million)
    assert sha(million).hex().startswith("e718483d0ce769644e2e42c7bc15b4638e1f98b13b2044285632a803afa973eb")


# ------------------------------------------------------------------ lengths, prefixes, splits
def test_every_total_length_as_a_single_part(emul):
    """1 .. 300 bytes as one part (a part has at least one byte; length 0 goes through the compression function alone, like
    every other length here): across the 111 / 112, 127 / 128 and 239 / 240 padding boundaries; aligned lengths in both
    forms, parts from an aligned and an odd address."""
    words = 0
    for total in range(0, 301):
        msg = HR.random_parts(1, [max(total, 1)], V.SEED + 0x4A00 + total)[0][0, :total].tobytes()
        assert HR.emul_stream(emul, msg) == sha(msg)
        if total:
            words += check_digests(emul, HR.random_parts(3, [total], V.SEED + 0x4A00 + total), b"", offsets=(0, 1))[0]
    assert words == 300 // 8                                                       # every multiple of 8 took the word form


@pytest.mark.parametrize("total", [130, 257])
@pytest.mark.parametrize("nparts", [1, 2, 3, 4])
def test_prefixes_and_part_boundaries_at_every_offset_of_a_block(emul, total, nparts):
    """Every prefix length of HR.PREFIX_LENS with the first part boundary at every byte offset of a block (the later boundaries
    one byte further each) for message totals of 130 and 257 bytes behind the prefix: 1, 2, 3 and 4 parts."""
    for plen in HR.PREFIX_LENS:
        prefix = HR.prefix_bytes(plen, plen)
        ats = [total] if nparts == 1 else range(1, min(128, total - (nparts - 1)) + 1)
        for at in ats:
            lens = [total] if nparts == 1 else HR.splits(total, nparts, at)
            assert len(lens) == nparts and sum(lens) == total
            parts = HR.random_parts(2, lens, V.SEED + 0x4B00 + 1000 * plen + at)
            check_digests(emul, parts, prefix, forms=("auto",) if at % 8 else ("auto", "bytes"))


def test_word_and_byte_form_agree(emul):
    """Aligned inputs (prefix 0 / 8 / 128 / 256, parts of multiples of 8 bytes) in both forms give identical output, for all
    three calls; the same parts from an odd address take the byte form; one row at the maximum of 65535 bytes."""
    for plen, lens in ((0, [8]), (8, [32, 32, 32]), (128, [8, 104]), (256, [112]), (0, [240]), (16, [96, 8, 8, 8]), (0, [1024])):
        prefix = HR.prefix_bytes(plen)
        parts = HR.random_parts(5, lens, V.SEED + 0x4C00 + plen + len(lens))
        assert check_digests(emul, parts, prefix, offsets=(0, 1, 3)) == [1, 0]
        for op in (1, 2):
            a, fa = HR.emul_rows(emul, op, parts, prefix)
            b, fb = HR.emul_rows(emul, op, parts, prefix, force_bytes=True)
            c, fc = HR.emul_rows(emul, op, parts, prefix, offset=1)
            assert (fa, fb, fc) == (1, 0, 0) and np.array_equal(a, b) and np.array_equal(a, c)
    big = HR.random_parts(1, [HR.MAX_ROW_BYTES], V.SEED + 0x4C80)
    check_digests(emul, big, b"", forms=("auto",), offsets=(0, 1))
    big = HR.random_parts(1, [HR.MAX_ROW_BYTES - 255 - 8, 8], V.SEED + 0x4C81)      # prefix + parts at the limit, byte form
    check_digests(emul, big, HR.prefix_bytes(255), forms=("auto",))
    big = HR.random_parts(1, [HR.MAX_ROW_BYTES - 256 - 7], V.SEED + 0x4C82)         # the longest row the word form takes: 65528
    assert check_digests(emul, big, HR.prefix_bytes(256)) == [1, 0]


def test_the_shared_vectors_all_pass(emul, oracle):
    assert HR.failures(emul, oracle) == []


# ------------------------------------------------------------------ the fused forms
def test_hash_to_scalar(emul):
    """2048 random rows of prefix(6) | 32 | 32 | 32: emul(sc_from_sha512) = emul(sc_from_bytes_wide)(hashlib digest) = the
    digest as a little-endian integer mod L.  Digests at the reduction's edge cases (0, L - 1, L, 2^256 - 1, 2^256, 2^512 - 1,
    multiples of L, every single bit) reach the fused tail as state words: no search for their messages."""
    prefix = HR.prefix_bytes(6)
    parts = HR.random_parts(2048, [32, 32, 32], V.SEED + 0x4D00)
    dig = HR.digests(parts, prefix)
    want = HR.scalars_of(dig)
    got, _ = HR.emul_rows(emul, 1, parts, prefix)
    composed = np.zeros((len(dig), 5), dtype=np.uint64)
    emul.emul_hash_sc_from_bytes_wide(C.c_void_p(dig.ctypes.data), C.c_void_p(composed.ctypes.data), C.c_size_t(len(dig)))
    assert np.array_equal(got, want) and np.array_equal(composed, want)
    assert (got[:, 4] < 1 << 41).all() and all(v < S.L for v in S.values(got[:16]))
    vals = S.reduction_values(64, 256, V.SEED + 0x4D01)
    assert 0 in vals and S.L in vals and 2**512 - 1 in vals and 2**262 * S.L in vals
    edges = S.to_bytes(vals, 64)
    assert np.array_equal(HR.emul_sc_from_state(emul, edges), S.canon_rows(vals))
    assert np.array_equal(HR.state_words(dig[:1])[0], np.frombuffer(dig[0].tobytes(), dtype=">u8").astype(np.uint64))


def test_hash_to_group(emul, oracle):
    """256 rows against the oracle's from_uniform_bytes of the hashlib digest, limb-exact; word and byte form."""
    for prefix, lens in ((HR.prefix_bytes(6), [32, 32, 32]), (b"", [64]), (HR.prefix_bytes(16), [7, 1])):
        parts = HR.random_parts(256 if len(lens) == 3 else 16, lens, V.SEED + 0x4E00 + len(lens))
        want = HR.points_of(HR.digests(parts, prefix))
        got, _ = HR.emul_rows(emul, 2, parts, prefix)
        assert np.array_equal(got, want)


# ------------------------------------------------------------------ the stand-alone sanitizer run
def _record(op, parts, prefix, want, force=0, offset=0):
    pad = lambda raw: raw + b"\0" * (-len(raw) % 8)
    lens = [p.shape[1] for p in parts]
    out = struct.pack("<6Q", op + 1, len(parts[0]), force, offset, len(prefix), len(parts)) + struct.pack("<%dQ" % len(lens), *lens)
    out += pad(bytes(prefix))
    for p in parts:
        out += pad(np.ascontiguousarray(p).tobytes())
    return out + pad(np.ascontiguousarray(want).tobytes())


def test_stand_alone_program_under_asan_and_ubsan(tmp_path, oracle):
    """tests/emul/hash_san.cpp with -fsanitize=address,undefined -fno-sanitize-recover=all and the bounds assertions, on a
    vector file of digests (both forms, parts ending with their heap block, aligned and odd), scalars and points; its exit
    status is the verdict."""
    exe = EB.sanitizer_program("hash_san.cpp", tmp_path, checked=True)
    blob, first = b"", None
    cases = [(b"", [t]) for t in (1, 7, 8, 111, 112, 119, 120, 127, 128, 129, 239, 240, 257)] + HR.kill_cases()[260:] + [(b"", [HR.MAX_ROW_BYTES])]
    for ci, (prefix, lens) in enumerate(cases):
        n = 1 if lens[0] > 4096 else 5
        parts = HR.random_parts(n, lens, V.SEED + 0x4F00 + ci)
        dig = HR.digests(parts, prefix)
        first = first if first is not None else (parts, dig)
        for force in ((0, 1) if HR.aligned(prefix, lens) else (1,)):
            for offset in ((0,) if not force else (0, 1, 7)):
                blob += _record(0, parts, prefix, dig, force, offset)
        blob += _record(1, parts, prefix, HR.scalars_of(dig))
        if ci % 4 == 0:
            blob += _record(2, parts, prefix, HR.points_of(dig))
    blob += struct.pack("<Q", 0)
    EB.assert_clean(EB.run_vectors(exe, blob, tmp_path, "vectors.bin"), "rows match")
    # the verdict is a real one: one expected byte changed and the program says so
    bad = bytearray(blob)
    parts, dig = first
    assert parts[0].shape == (5, 1)
    bad[7 * 8 + 0 + 8 + 64 * 3 + 9] ^= 1           # header (6 words + 1 length), empty prefix, the part (5 bytes padded to 8): byte 9 of row 3
    EB.assert_caught(EB.run_vectors(exe, bad, tmp_path, "wrong.bin"), "record 0 (op 0): row 3 byte 9")
