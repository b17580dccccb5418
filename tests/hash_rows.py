"""Messages and expected values for zc_sha512_rows, zc_sc_from_sha512 and zc_ris_from_sha512, shared by the CPU emulation tier,
the planted-defect catalogue and the GPU tier (this module holds no test).

A case is (prefix bytes, [part lengths]); its rows are seeded random bytes.  Expected digests come from hashlib.sha512, expected
scalars are int.from_bytes(digest, "little") mod L as canonical limbs (tests/scalar_ext_rows.canon_rows), expected points are the
oracle's ris_from_uniform_bytes of the digest.  The round constants and initial values are DERIVED here from the primes with
exact integer arithmetic, so that the header's table is not compared with a second typed-in copy."""
import hashlib

import numpy as np

from tests import scalar_ext_rows as S

MAX_PARTS, MAX_PREFIX, MAX_ROW_BYTES = 4, 256, 65535
M64 = (1 << 64) - 1


# ------------------------------------------------------------------ the constants, from the primes
def first_primes(k):
    out, c = [], 2
    while len(out) < k:
        if all(c % q for q in out if q * q <= c):
            out.append(c)
        c += 1
    return out


def iroot(v, k):
    """floor(v^(1/k)) for k = 2, 3, exact: Newton from above, then settled by comparison."""
    x = 1 << -(-v.bit_length() // k)
    while True:
        y = ((k - 1) * x + v // x ** (k - 1)) // k
        if y >= x:
            break
        x = y
    while x ** k > v:
        x -= 1
    while (x + 1) ** k <= v:
        x += 1
    return x


def round_constants():
    """The first 64 fractional bits of the cube roots of the first 80 primes: floor(p^(1/3) 2^64) mod 2^64."""
    return [iroot(p << 192, 3) & M64 for p in first_primes(80)]


def initial_values():
    """The same of the square roots of the first 8 primes."""
    return [iroot(p << 128, 2) & M64 for p in first_primes(8)]


# ------------------------------------------------------------------ rows and expectations
def random_parts(n, lens, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=(n, l), dtype=np.uint8) for l in lens]


def messages(parts, prefix=b""):
    n = len(parts[0])
    assert all(len(p) == n and p.dtype == np.uint8 for p in parts)
    return [bytes(prefix) + b"".join(p[i].tobytes() for p in parts) for i in range(n)]


def digests(parts, prefix=b""):
    msgs = messages(parts, prefix)
    return np.frombuffer(b"".join(hashlib.sha512(m).digest() for m in msgs), dtype=np.uint8).reshape(len(msgs), 64).copy()


def scalars_of(dig):
    """(n, 5) canonical limbs of the digests read as little-endian 512-bit integers mod L."""
    return S.canon_rows([int.from_bytes(d.tobytes(), "little") for d in dig])


def points_of(dig):
    from oracle import zc_ref
    return zc_ref.ris_from_uniform_bytes(dig)


def prefix_bytes(k, seed=0):
    return bytes((seed + 7 * i + 1) & 0xFF for i in range(k))


def splits(total, nparts, at):
    """`total` bytes cut into nparts parts with the first boundary at byte `at` (1 <= at), the later ones one and two bytes
    further: [at, 1, 1, rest] for four parts."""
    cuts = [at] + [1] * (nparts - 2) if nparts > 1 else []
    rest = total - sum(cuts)
    assert rest >= 1, (total, nparts, at)
    return cuts + [rest]


# ------------------------------------------------------------------ state words for given digests (the fused forms' last step)
def state_words(dig):
    """The eight big-endian state words whose digest is each 64-byte row."""
    return np.ascontiguousarray(np.asarray(dig, dtype=np.uint8)).view(">u8").astype(np.uint64)


# ------------------------------------------------------------------ the vectors a planted defect must not survive
PREFIX_LENS = [0, 1, 7, 8, 111, 112, 127, 128, 129, 255, 256]
FIPS_ABC = b"abc"
FIPS_TWO_BLOCKS = b"abcdefghbcdefghicdefghijdefghijkefghijklfghijklmghijklmnhijklmnoijklmnopjklmnopqklmnopqrlmnopqrsmnopqrstnopqrstu"


OUT_BYTES = {0: 64, 1: 40, 2: 160}                   # op 0: digest, 1: five limbs, 2: twenty limbs


def emul_rows(lib, op, parts, prefix=b"", force_bytes=False, offset=0):
    """tests/emul/hash_emul.cpp's emul_hash_rows on copies of the parts that start `offset` bytes past an 8-byte boundary.
    Returns (output rows: (n, 64) uint8 or (n, 5 / 20) uint64, 1 when the word form ran, 0 for the byte form)."""
    import ctypes as C
    n = len(parts[0])
    keep, ptrs = [], []
    for p in parts:
        buf = np.zeros(p.size + 16, dtype=np.uint8)
        start = -buf.ctypes.data % 8 + offset
        buf[start:start + p.size] = p.reshape(-1)
        keep.append(buf)
        ptrs.append(buf.ctypes.data + start)
    out = np.zeros((n, OUT_BYTES[op]), dtype=np.uint8)
    k = len(parts)
    form = lib.emul_hash_rows(op, bytes(prefix), C.c_size_t(len(prefix)), (C.c_void_p * k)(*ptrs), (C.c_size_t * k)(*[p.shape[1] for p in parts]), C.c_size_t(k),
                              C.c_void_p(out.ctypes.data), C.c_size_t(n), 1 if force_bytes else 0)
    assert form in (0, 1), form
    return (out if op == 0 else out.view(np.uint64)), form


def emul_stream(lib, msg):
    import ctypes as C
    out = np.zeros(64, dtype=np.uint8)
    lib.emul_sha512_stream(bytes(msg), C.c_size_t(len(msg)), C.c_void_p(out.ctypes.data))
    return out.tobytes()


def emul_tables(lib):
    import ctypes as C
    k, iv = np.zeros(80, dtype=np.uint64), np.zeros(8, dtype=np.uint64)
    lib.emul_sha512_tables(C.c_void_p(k.ctypes.data), C.c_void_p(iv.ctypes.data))
    return [int(x) for x in k], [int(x) for x in iv]


def emul_sc_from_state(lib, dig):
    import ctypes as C
    st = state_words(dig)
    out = np.zeros((len(st), 5), dtype=np.uint64)
    lib.emul_sc_from_state(C.c_void_p(st.ctypes.data), C.c_void_p(out.ctypes.data), C.c_size_t(len(st)))
    return out


def aligned(prefix, lens):
    return len(prefix) % 8 == 0 and all(l % 8 == 0 for l in lens)


def failures(lib, oracle=None, rows=3):
    """Every vector of this module on one build of tests/emul/hash_emul.cpp: the labels "<family> [<case>]" of those that do not
    give the expected value.  Families: tables, stream, digest word, digest bytes, scalar, scalar edges, point."""
    bad = []
    if emul_tables(lib) != (round_constants(), initial_values()):
        bad.append("tables [k, iv]")
    for name, msg in (("abc", FIPS_ABC), ("two blocks", FIPS_TWO_BLOCKS), ("empty", b"")):
        if emul_stream(lib, msg) != hashlib.sha512(msg).digest():
            bad.append("stream [%s]" % name)
    for ci, (prefix, lens) in enumerate(kill_cases()):
        parts = random_parts(rows, lens, 0x4A5B0000 + ci)
        want = digests(parts, prefix)
        case = "prefix=%d parts=%s" % (len(prefix), ",".join(map(str, lens)))
        for force in ([False, True] if aligned(prefix, lens) else [True]):
            got, form = emul_rows(lib, 0, parts, prefix, force_bytes=force)
            assert form == (0 if force else 1), (case, force, form)
            if not np.array_equal(got, want):
                bad.append("digest %s [%s]" % ("bytes" if force else "word", case))
        if len(lens) > 1 or lens[0] % 50 == 0:
            if not np.array_equal(emul_rows(lib, 1, parts, prefix)[0], scalars_of(want)):
                bad.append("scalar [%s]" % case)
        if oracle is not None and lens == [32, 32, 32]:
            if not np.array_equal(emul_rows(lib, 2, parts, prefix)[0], oracle.ris_from_uniform_bytes(want)):
                bad.append("point [%s]" % case)
    edges = S.to_bytes(S.reduction_values(64, 64, 0x4A5C0001), 64)
    if not np.array_equal(emul_sc_from_state(lib, edges), scalars_of(edges)):
        bad.append("scalar edges [wide_edges, single bits, random]")
    return bad


def kill_cases():
    """[(prefix, part lengths)]: every message length 1 .. 260 as one part -- the 111 / 112, 127 / 128 and 239 / 240 padding
    boundaries among them, and the aligned lengths that take the word form -- then prefixes and several parts, in both forms."""
    cases = [(b"", [t]) for t in range(1, 261)]
    cases += [(prefix_bytes(6), [32, 32, 32]), (prefix_bytes(8), [32, 32, 32]), (prefix_bytes(128), [8, 104]), (prefix_bytes(5), [5, 3, 120, 1]),
              (prefix_bytes(256), [112]), (b"", [240]), (prefix_bytes(16), [96]), (prefix_bytes(7), [104, 1])]
    return cases
