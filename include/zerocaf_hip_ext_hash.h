/*
 * zerocaf_hip_ext_hash.h -- additive entry points beyond the 0.6 table: SHA-512 over batched rows, and the hash-to-scalar and
 * hash-to-group calls that consume the digest without writing it to memory.
 *
 * Part of zerocaf_hip_ext.h, which includes this file: a caller includes that header (or this one alone) and finds the
 * declarations below.  Same libraries and conventions as everything in zerocaf_hip.h (status codes, host or device arrays, the
 * context's stream); zc_version() stays as it is.  Plain C11.
 */
#ifndef ZEROCAF_HIP_EXT_HASH_H
#define ZEROCAF_HIP_EXT_HASH_H

#include "zerocaf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZC_HASH_MAX_PARTS      4
#define ZC_HASH_MAX_PREFIX     256
#define ZC_HASH_MAX_ROW_BYTES  65535     /* prefix_len + sum of part_len */

/* The message of row i is M_i = prefix || parts[0][i] || parts[1][i] || ... || parts[nparts-1][i]: what a Schnorr challenge
 * SHA-512(domain || R_i || A_i || m_i) or a hash-to-group of per-row inputs needs, with R, A and m left where the calls that
 * made them put them.
 *
 *   - prefix is the domain separator or the common transcript, the same prefix_len bytes for every row.  It is ALWAYS HOST
 *     memory, at most ZC_HASH_MAX_PREFIX (256) bytes, copied during the call; it may be NULL only when prefix_len == 0.
 *   - parts and part_len are host arrays of nparts entries (1 .. ZC_HASH_MAX_PARTS), read during the call.  parts[j] holds n rows
 *     of part_len[j] contiguous bytes (the stride equals the length), part_len[j] is 1 .. 65535.  Every row of a call has the
 *     same length prefix_len + sum of part_len, at most ZC_HASH_MAX_ROW_BYTES (65535).
 *
 * zc_sha512_rows:     out64[i] = the 64 bytes of SHA-512(M_i) in FIPS 180-4 byte order.
 * zc_sc_from_sha512:  out[i] = exactly zc_sc_from_bytes_wide of those 64 bytes: the digest read as a little-endian 512-bit integer
 *                     mod L, five canonical limbs.  Fused: no digest reaches memory.
 * zc_ris_from_sha512: out[i] = exactly zc_ris_from_uniform_bytes of those 64 bytes (src/ristretto.rs:493-507), the same 20 limbs.
 *                     Fused likewise.
 *
 *   - ZC_ERR_BAD_ARG before the context is touched, in this order: parts NULL ("null pointer: parts"); part_len NULL ("null
 *     pointer: part_len"); the output NULL, by its name ("null pointer: out64" / "null pointer: out"); prefix NULL with prefix_len
 *     > 0 ("null pointer: prefix"); nparts outside 1 .. 4; a parts[j] NULL ("null pointer: parts[j]" with the index); a part_len[j]
 *     of 0; prefix_len > 256; a row longer than 65535 bytes; n * part_len[j] overflowing size_t; then the context ("null
 *     context").
 *   - n == 0: ZC_OK, nothing written; checked after the pointer and limit checks.
 *   - All parts[j] and the output in host memory (staged in chunks, synchronous, sharded over the devices of a multi-device
 *     context like zc_sc_from_bytes_wide) or all on one device of the context (used in place, asynchronous on the context's
 *     stream); anything else is ZC_ERR_MIXED_MEM.
 *   - Device byte arrays -- the parts and out64 -- need no alignment: an odd address works.  The limb outputs need 8-byte
 *     alignment.  Parts that are all multiples of 8 bytes long at addresses that are multiples of 8, behind a prefix of a
 *     multiple of 8 bytes, are read eight bytes at a time; the result does not depend on it.
 *   - The output must not overlap a part.  The call writes rows 0 .. n-1 of the output and nothing else, and no byte of any input.
 *   - No environment knob. */
int zc_sha512_rows(zc_ctx *ctx, const uint8_t *prefix, size_t prefix_len, const uint8_t *const *parts,
                   const size_t *part_len, size_t nparts, uint8_t *out64, size_t n);
int zc_sc_from_sha512(zc_ctx *ctx, const uint8_t *prefix, size_t prefix_len, const uint8_t *const *parts,
                      const size_t *part_len, size_t nparts, uint64_t *out, size_t n);       /* n x 5 limbs  */
int zc_ris_from_sha512(zc_ctx *ctx, const uint8_t *prefix, size_t prefix_len, const uint8_t *const *parts,
                       const size_t *part_len, size_t nparts, uint64_t *out, size_t n);      /* n x 20 limbs */

#ifdef __cplusplus
}
#endif

#endif /* ZEROCAF_HIP_EXT_HASH_H */
