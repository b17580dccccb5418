// zc_hash.hip.h -- SHA-512 (FIPS 180-4) over batched rows, one row per lane, and the two calls that consume the digest in
// registers: hash-to-scalar (sc_reduce_words) and hash-to-group (ris_from_uniform_words).
//
// A row's message is M_i = prefix || parts[0][i] || parts[1][i] || ...: the prefix is the same for every row and travels in the
// kernel's argument block, part j is n rows of part_len[j] contiguous bytes.  Every row of a launch has the same length, so the
// number of 128-byte blocks, every padding decision and every part boundary is wave-uniform: the reader's branches are scalar
// branches and the block loop never diverges.
//
// Why this shape on gfx950:
//   * the message schedule is a rolling w[16] and the 80 rounds run as five groups of 16 with every index a compile-time
//     constant: state (16 VGPRs), schedule (32) and a dozen temporaries stay in registers.  A w[] indexed at run time would
//     live in scratch;
//   * the round constants sit in __constant__ memory and are read at wave-uniform addresses: scalar loads, no VGPR, no LDS;
//   * a 64-bit rotate is two 32-bit funnel shifts (v_alignbit_b32), half the cost of the shift / shift / or triple on 64-bit
//     registers;
//   * with stride = length the rows of a wave are adjacent in memory, so the lanes' own loads cover whole cache lines between
//     them and nothing is staged through LDS.
// The per-lane functions compile for the host as well (tests/emul/hash_emul.cpp); the kernels follow when this file comes in
// after zc_kernels.hip.h.
#pragma once
#include "zc_curve.hip.h"

namespace zc {

constexpr int HASH_MAX_PARTS = 4;
constexpr u32 HASH_MAX_PREFIX = 256;
constexpr u32 HASH_MAX_ROW_BYTES = 65535;

// One launch's messages, passed to the kernels by value.
struct HashMsg {
    const uint8_t* part[HASH_MAX_PARTS];   // n rows of part_len[j] bytes each (device memory)
    u32 part_len[HASH_MAX_PARTS];
    u32 nparts;
    u32 prefix_len;
    u32 total;                             // prefix_len + sum of part_len: bytes per row, at most HASH_MAX_ROW_BYTES
    u32 words;                             // nonzero: prefix_len, every part_len and every part address are multiples of 8
    u64 prefix[HASH_MAX_PREFIX / 8];       // the prefix bytes in memory order (byte k = bits 8 (k mod 8) of word k / 8), zero beyond
};

// Round constants: the first 64 fractional bits of the cube roots of the first 80 primes; initial state: the same of the
// square roots of the first 8 (FIPS 180-4, 4.2.3 and 5.3.5).  tests/hash_rows.py derives both from the primes.
struct sha512_tables {
    u64 k[80];
    u64 iv[8];
};
__device__ __constant__ sha512_tables ZC_SHA512 = {
    {0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull, 0x3956c25bf348b538ull, 0x59f111f1b605d019ull,
     0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull, 0xd807aa98a3030242ull, 0x12835b0145706fbeull, 0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull,
     0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull, 0xc19bf174cf692694ull, 0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull,
     0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull, 0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull,
     0x983e5152ee66dfabull, 0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull, 0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull,
     0x06ca6351e003826full, 0x142929670a0e6e70ull, 0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull, 0x53380d139d95b3dfull,
     0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull, 0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull,
     0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull, 0xd192e819d6ef5218ull, 0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull,
     0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull, 0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull, 0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull,
     0x5b9cca4f7763e373ull, 0x682e6ff3d6b2b8a3ull, 0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
     0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull, 0xca273eceea26619cull, 0xd186b8c721c0c207ull,
     0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull, 0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull, 0x113f9804bef90daeull, 0x1b710b35131c471bull,
     0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull, 0x431d67c49c100d4cull, 0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull,
     0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull},
    {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull, 0x510e527fade682d1ull, 0x9b05688c2b3e6c1full,
     0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull}};

// ---------------------------------------------------------------- the compression function
// x rotated right by N bits, 0 < N < 64 and N != 32: each half of the result is one funnel shift over the two halves of x.
template <int N>
ZC_DI u64 rotr64(u64 x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const u32 lo = (u32)x, hi = (u32)(x >> 32);
    const u32 a = N < 32 ? lo : hi, b = N < 32 ? hi : lo;                    // the result's low half starts in a, its high half in b
    const u32 rl = __builtin_amdgcn_alignbit(b, a, N & 31), rh = __builtin_amdgcn_alignbit(a, b, N & 31);
    return (u64)rh << 32 | rl;
#else
    return x >> N | x << (64 - N);
#endif
}
ZC_DI u64 sha512_Sigma0(u64 x) { return rotr64<28>(x) ^ rotr64<34>(x) ^ rotr64<39>(x); }
ZC_DI u64 sha512_Sigma1(u64 x) { return rotr64<14>(x) ^ rotr64<18>(x) ^ rotr64<41>(x); }
ZC_DI u64 sha512_sigma0(u64 x) { return rotr64<1>(x) ^ rotr64<8>(x) ^ (x >> 7); }
ZC_DI u64 sha512_sigma1(u64 x) { return rotr64<19>(x) ^ rotr64<61>(x) ^ (x >> 6); }
ZC_DI u64 sha512_ch(u64 e, u64 f, u64 g) { return g ^ (e & (f ^ g)); }
ZC_DI u64 sha512_maj(u64 a, u64 b, u64 c) { return (a & b) | (c & (a | b)); }

// Rounds r0 .. r0 + 15 on the working variables v[0..7] = a..h.  The variables do not move: round j reads them through
// indices rotated by j, all compile-time constants, and after 16 rounds the rotation is back where it started.  SCHED: the
// schedule word of round t >= 16 replaces w[t mod 16] first.
template <bool SCHED>
ZC_DI void sha512_rounds16(u64 (&v)[8], u64 (&w)[16], const u64* __restrict__ k)
{
#pragma unroll
    for (int j = 0; j < 16; j++) {
        if (SCHED) w[j] += sha512_sigma1(w[(j + 14) & 15]) + w[(j + 9) & 15] + sha512_sigma0(w[(j + 1) & 15]);
        u64 &a = v[(0 - j) & 7], &b = v[(1 - j) & 7], &c = v[(2 - j) & 7], &d = v[(3 - j) & 7];
        u64 &e = v[(4 - j) & 7], &f = v[(5 - j) & 7], &g = v[(6 - j) & 7], &h = v[(7 - j) & 7];
        const u64 t1 = h + sha512_Sigma1(e) + sha512_ch(e, f, g) + k[j] + w[j];
        const u64 t2 = sha512_Sigma0(a) + sha512_maj(a, b, c);
        d += t1;
        h = t1 + t2;
    }
}
// state <- state + compress(state, block); w holds the block's sixteen big-endian words and is used up as the schedule.
ZC_DI void sha512_compress(u64 (&state)[8], u64 (&w)[16])
{
    u64 v[8];
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = state[i];
    sha512_rounds16<false>(v, w, ZC_SHA512.k);
#pragma unroll 1
    for (int r = 16; r < 80; r += 16) sha512_rounds16<true>(v, w, ZC_SHA512.k + r);
#pragma unroll
    for (int i = 0; i < 8; i++) state[i] += v[i];
}
ZC_DI void sha512_init(u64 (&state)[8])
{
#pragma unroll
    for (int i = 0; i < 8; i++) state[i] = ZC_SHA512.iv[i];
}

// ---------------------------------------------------------------- the message reader
// Blocks of a message of `total` bytes: the 0x80 marker and the 16-byte length must fit behind the data of the last one.
ZC_DI u32 hash_blocks(u32 total) { return (total >> 7) + 1 + ((total & 127) > 111 ? 1 : 0); }

ZC_DI u64 hash_load8_aligned(const uint8_t* p) { return *reinterpret_cast<const u64*>(p); }
ZC_DI u64 hash_load8_any(const uint8_t* p)
{
    u64 x;
    __builtin_memcpy(&x, p, 8);              // no alignment promise: global memory takes unaligned accesses
    return x;
}

// WORD FORM (m.words): the eight message bytes from `pos` on, a multiple of 8 at or below m.total, as a big-endian word --
// one 8-byte load, or the marker when the data ends here.
ZC_DI u64 hash_word_aligned(const HashMsg& m, size_t i, u32 pos)
{
    if (pos == m.total) return 0x8000000000000000ull;
    if (pos < m.prefix_len) return __builtin_bswap64(m.prefix[pos >> 3]);
    u32 off = pos - m.prefix_len;
#pragma unroll
    for (int j = 0; j < HASH_MAX_PARTS; j++) {
        if (j >= (int)m.nparts) break;
        if (off < m.part_len[j]) return __builtin_bswap64(hash_load8_aligned(m.part[j] + i * m.part_len[j] + off));
        off -= m.part_len[j];
    }
    return 0;
}

// BYTE FORM: any lengths, any addresses.  Byte `pos` < m.total of row i:
ZC_DI u32 hash_byte(const HashMsg& m, size_t i, u32 pos)
{
    if (pos < m.prefix_len) return (u32)(m.prefix[pos >> 3] >> (8 * (pos & 7))) & 0xFFu;
    u32 off = pos - m.prefix_len;
#pragma unroll
    for (int j = 0; j < HASH_MAX_PARTS; j++) {
        if (j >= (int)m.nparts) break;
        if (off < m.part_len[j]) return m.part[j][i * m.part_len[j] + off];
        off -= m.part_len[j];
    }
    return 0;
}
// the same word as hash_word_aligned, pos a multiple of 8 at or below m.total: eight bytes of one part come in with one
// unaligned load, a word that crosses a boundary (prefix / part / end of data) is put together byte by byte.
ZC_DI u64 hash_word_bytes(const HashMsg& m, size_t i, u32 pos)
{
    if (pos + 8 <= m.prefix_len) return __builtin_bswap64(m.prefix[pos >> 3]);
    if (pos + 8 <= m.total && pos >= m.prefix_len) {
        u32 off = pos - m.prefix_len;
#pragma unroll
        for (int j = 0; j < HASH_MAX_PARTS; j++) {
            if (j >= (int)m.nparts) break;
            if (off < m.part_len[j]) {
                if (off + 8 <= m.part_len[j]) return __builtin_bswap64(hash_load8_any(m.part[j] + i * m.part_len[j] + off));
                break;
            }
            off -= m.part_len[j];
        }
    }
    u64 w = 0;
#pragma unroll 1                             // a few words per block come here.  Kept a loop: unrolled in all sixteen words it makes k_sha512_rows 67 KB of code, so 32 KB
    for (u32 k = 0; k < 8; k++) {
        const u32 p = pos + k;
        const u32 byte = p < m.total ? hash_byte(m, i, p) : p == m.total ? 0x80u : 0u;
        w = w << 8 | byte;
    }
    return w;
}
// The sixteen big-endian words of block b of M_i, padding and length field included.  WORDS selects the form; both give the
// same words wherever the word form applies.
template <bool WORDS>
ZC_DI void hash_read_block(u64 (&w)[16], const HashMsg& m, size_t i, u32 b, u32 nblocks)
{
#pragma unroll
    for (int t = 0; t < 16; t++) {
        const u32 pos = 128 * b + 8 * (u32)t;
        u64 x = 0;
        if (pos <= m.total) x = WORDS ? hash_word_aligned(m, i, pos) : hash_word_bytes(m, i, pos);
        // the 128-bit length in bits: its high word and everything above bit 19 of the low one are zero (total <= 65535)
        if (t == 15 && b + 1 == nblocks) x = (u64)m.total * 8;
        w[t] = x;
    }
}
// SHA-512(M_i) as the eight state words (big-endian words of the digest).
ZC_DI void sha512_row(u64 (&state)[8], const HashMsg& m, size_t i)
{
    sha512_init(state);
    const u32 nblocks = hash_blocks(m.total);
#pragma unroll 1
    for (u32 b = 0; b < nblocks; b++) {
        u64 w[16];
        if (m.words) hash_read_block<true>(w, m, i, b, nblocks);
        else hash_read_block<false>(w, m, i, b, nblocks);
        sha512_compress(state, w);
    }
}

// ---------------------------------------------------------------- what the three calls do with the state
// the digest's 64 bytes in FIPS order, through 8-byte stores that promise no alignment
ZC_DI void sha512_store_digest(uint8_t* out, const u64 (&state)[8])
{
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const u64 x = __builtin_bswap64(state[k]);
        __builtin_memcpy(out + 8 * k, &x, 8);
    }
}
// the digest bytes read as a little-endian 512-bit integer lo + 2^256 hi (what zc_sc_from_bytes_wide and
// zc_ris_from_uniform_bytes load from memory): byte 8 k + b of the digest is bits 56 - 8 b of state word k
ZC_DI void sha512_digest_words(u64 (&lo)[4], u64 (&hi)[4], const u64 (&state)[8])
{
    u64 d[8];
#pragma unroll
    for (int k = 0; k < 8; k++) d[k] = __builtin_bswap64(state[k]);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        lo[k] = d[k];
        hi[k] = d[4 + k];
    }
}
// out = int.from_bytes(SHA-512(M_i), "little") mod L, five canonical limbs: zc_sc_from_bytes_wide on a digest that never
// reaches memory
ZC_DI void sc_from_sha512_row(u64* out, const HashMsg& m, size_t i)
{
    u64 state[8], lo[4], hi[4], l[5];
    sha512_row(state, m, i);
    sha512_digest_words(lo, hi, state);
    fe_to_limbs52(l, sc_reduce_words<true>(lo, hi));
    store5(out, l);
}
// out = from_uniform_bytes(SHA-512(M_i)) (ristretto.rs:493-507), 20 canonical limbs: zc_ris_from_uniform_bytes likewise
ZC_DI void ris_from_sha512_row(u64* out, const HashMsg& m, size_t i)
{
    u64 state[8], lo[4], hi[4];
    sha512_row(state, m, i);
    sha512_digest_words(lo, hi, state);
    pt_store(out, ris_from_uniform_words(lo, hi));
}

// ---------------------------------------------------------------- kernels: one row per lane, ZC_BLOCK threads
#ifdef ZC_KERNEL
// The message description is the kernels' FIRST parameter and is read where the launch put it, in the kernel's argument
// block: the prefix words are indexed by the block counter, and a by-value parameter indexed at run time is otherwise
// copied to scratch first (328 bytes per lane).  From the argument block every field and every prefix word is a scalar load.
ZC_DI const HashMsg& hash_msg_in_argument_block(const HashMsg& first_parameter)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const HashMsg __attribute__((address_space(4))) * arg_ptr;
    (void)first_parameter;
    return *(const HashMsg*)(arg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
#else
    return first_parameter;
#endif
}
ZC_KERNEL void k_sha512_rows(const HashMsg m, uint8_t* out, size_t n)
{
    const size_t i = gid();
    if (i >= n) return;
    u64 state[8];
    sha512_row(state, hash_msg_in_argument_block(m), i);
    sha512_store_digest(out + 64 * i, state);
}
ZC_KERNEL void k_sc_from_sha512(const HashMsg m, u64* out, size_t n)
{
    const size_t i = gid();
    if (i >= n) return;
    sc_from_sha512_row(out + 5 * i, hash_msg_in_argument_block(m), i);
}
// (Elligator's register budget, as k_ris_from_uniform_bytes)
ZC_KERNEL_2W void k_ris_from_sha512(const HashMsg m, u64* out, size_t n)
{
    const size_t i = gid();
    if (i >= n) return;
    ris_from_sha512_row(out + 20 * i, hash_msg_in_argument_block(m), i);
}
#endif

}  // namespace zc
