// hash_emul.cpp -- TEST-ONLY host build of the per-lane functions behind zc_sha512_rows, zc_sc_from_sha512 and zc_ris_from_sha512
// (zc_hash.hip.h: sha512_compress, the message reader in its word and byte forms, sha512_row and what the three kernels do with
// the state).  The loop over i stands for the launch of k_sha512_rows / k_sc_from_sha512 / k_ris_from_sha512: one call per lane,
// with the message description built as hash_rows_call (zerocaf_hip.hip) builds it.  Never shipped.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../dusk_zerocaf_amd/csrc/zc_hash.hip.h"

extern "C" void zc_bound_fail(const char* what, int line)
{
    std::fprintf(stderr, "zc_arith.hip.h:%d: bound violated: %s\n", line, what);
    std::abort();
}

using namespace zc;

extern "C" {
// the header's tables as the device reads them: 80 round constants, 8 initial values
void emul_sha512_tables(u64* k80, u64* iv8)
{
    for (int i = 0; i < 80; i++) k80[i] = ZC_SHA512.k[i];
    for (int i = 0; i < 8; i++) iv8[i] = ZC_SHA512.iv[i];
}
// sha512_init / sha512_compress alone over a message of any length (the padding is done here, not by the reader)
void emul_sha512_stream(const uint8_t* msg, size_t len, uint8_t* out64)
{
    u64 state[8];
    sha512_init(state);
    const size_t nblocks = (len + 17 + 127) / 128;
    for (size_t b = 0; b < nblocks; b++) {
        uint8_t blk[128] = {0};
        for (size_t k = 0; k < 128; k++) {
            const size_t pos = 128 * b + k;
            blk[k] = pos < len ? msg[pos] : pos == len ? 0x80 : 0;
        }
        if (b + 1 == nblocks)
            for (int k = 0; k < 8; k++) blk[120 + k] = (uint8_t)(((u64)len * 8) >> (56 - 8 * k));
        u64 w[16];
        for (int t = 0; t < 16; t++) {
            w[t] = 0;
            for (int k = 0; k < 8; k++) w[t] = w[t] << 8 | blk[8 * t + k];
        }
        sha512_compress(state, w);
    }
    sha512_store_digest(out64, state);
}
// op 0: n x 64 digest bytes, 1: n x 5 limbs, 2: n x 20 limbs.  force_bytes: the byte form also where the word form applies.
// Returns 1 when the word form ran, 0 for the byte form, -1 for arguments the library would refuse.
int emul_hash_rows(int op, const uint8_t* prefix, size_t prefix_len, const uint8_t* const* parts, const size_t* part_len, size_t nparts, void* out,
                   size_t n, int force_bytes)
{
    if (nparts < 1 || nparts > (size_t)HASH_MAX_PARTS || prefix_len > HASH_MAX_PREFIX) return -1;
    HashMsg m = {};
    m.nparts = (u32)nparts;
    m.prefix_len = (u32)prefix_len;
    size_t total = prefix_len;
    bool words = prefix_len % 8 == 0;
    if (prefix_len) std::memcpy(m.prefix, prefix, prefix_len);
    for (size_t j = 0; j < nparts; j++) {
        if (part_len[j] == 0 || part_len[j] > HASH_MAX_ROW_BYTES - total) return -1;
        total += part_len[j];
        m.part[j] = parts[j];
        m.part_len[j] = (u32)part_len[j];
        words = words && part_len[j] % 8 == 0 && reinterpret_cast<uintptr_t>(parts[j]) % 8 == 0;
    }
    m.total = (u32)total;
    m.words = words && !force_bytes ? 1 : 0;
    for (size_t i = 0; i < n; i++) {
        if (op == 0) {
            u64 state[8];
            sha512_row(state, m, i);
            sha512_store_digest(static_cast<uint8_t*>(out) + 64 * i, state);
        } else if (op == 1) {
            sc_from_sha512_row(static_cast<u64*>(out) + 5 * i, m, i);
        } else {
            ris_from_sha512_row(static_cast<u64*>(out) + 20 * i, m, i);
        }
    }
    return (int)m.words;
}
// the last step of k_sc_from_sha512 on given state words (n x 8): digests of any value reach the reduction without a search
// for their messages
void emul_sc_from_state(const u64* state, u64* out, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        u64 s[8], lo[4], hi[4], l[5];
        for (int k = 0; k < 8; k++) s[k] = state[8 * i + k];
        sha512_digest_words(lo, hi, s);
        fe_to_limbs52(l, sc_reduce_words<true>(lo, hi));
        store5(out + 5 * i, l);
    }
}
// zc_sc_from_bytes_wide's own function on digests from elsewhere (as tests/emul/scalar_ext_emul.cpp)
void emul_hash_sc_from_bytes_wide(const uint8_t* in, u64* out, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        u64 lo[4], hi[4], l[5];
        for (int k = 0; k < 4; k++) {
            std::memcpy(&lo[k], in + 64 * i + 8 * k, 8);
            std::memcpy(&hi[k], in + 64 * i + 32 + 8 * k, 8);
        }
        fe_to_limbs52(l, sc_reduce_words<true>(lo, hi));
        store5(out + 5 * i, l);
    }
}
}
