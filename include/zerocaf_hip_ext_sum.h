/*
 * zerocaf_hip_ext_sum.h -- additive entry points beyond the 0.6 table that reduce a whole batch to one result.
 *
 * Part of zerocaf_hip_ext.h, which includes this file: a caller includes that header (or this one alone) and finds the
 * declarations below.  Same libraries and conventions as everything in zerocaf_hip.h (status codes, host or device arrays, the
 * context's stream, zero decided by value); zc_version() stays as it is.  Plain C11.
 */
#ifndef ZEROCAF_HIP_EXT_SUM_H
#define ZEROCAF_HIP_EXT_SUM_H

#include "zerocaf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The weighted sum of ALL rows of a wire-format batch as one multi-scalar multiplication: what a batch verifier (Schnorr
 * signatures, DLEQ proofs, Bulletproofs) checks against the identity, where zc_ris_lincomb pays a doubling chain per row.
 *
 * out32 = compress( b * RISTRETTO_BASEPOINT + sum_{i<n, ok_i} sum_{j<terms} w_ij * decompress(in32[i][j]) )
 *   w_ij = val(weights[i]) * val(scalars[i][j]) mod L            (weights == NULL: val(scalars[i][j]) mod L)
 *   b    = sum_{i<n, ok_i} val(weights[i]) * val(base_scalars[i]) mod L   (base_scalars == NULL: no base term)
 *   ok_i = every one of row i's `terms` encodings decodes (src/ristretto.rs:96-154)
 *
 *   - Layouts as zc_ris_lincomb: in32 n x terms x 32 bytes, row-major; scalars n x terms x 5 limbs; base_scalars and weights
 *     NULL or n x 5 limbs; ok NULL or n bytes.  out32 is 32 bytes in HOST memory, like zc_msm's out_point: the call is
 *     synchronous.  With weights == NULL, base_scalars == NULL and terms == 1 this is the plain MSM over encodings.
 *   - Every scalar and weight is read BY VALUE, as the scalar operations for protocols read them: val(w) = sum (w_i mod 2^52)
 *     2^(52 i), reduced mod L.  (Not the loop-test rule of zc_ris_lincomb's double_and_add; for canonical operands below L
 *     the two agree.)  A subtracted term is k = L - c; weights of 128 random bits suffice for batch verification.
 *   - The 32 bytes are the reference's compress of the sum built with its Mul<Scalar> and + from the canonical w_ij and b: an
 *     encoding depends on the group element only.
 *   - A row with an undecodable term gets ok[i] = 0 and is left out completely -- its terms and its share of b, whatever its
 *     scalars and its weight; no other row's contribution changes.  Every other row gets ok[i] = 1.
 *   - All rows rejected, or a sum that is the identity: 32 zero bytes.  n == 0: ZC_OK and 32 zero bytes, the empty sum.
 *     A caller verifies with: every ok is 1 and out32 is 32 zero bytes.
 *   - ZC_ERR_BAD_ARG before anything is touched: in32, scalars or out32 NULL ("null pointer: in32", ...), checked before
 *     everything else; terms == 0; n * terms + 1 >= 2^31, or any other limit at which zc_msm refuses a shard of that many
 *     pairs; then the context ("null context").
 *   - in32, scalars, base_scalars, weights and ok all in host memory (staged on device slot 0, as zc_msm_batch stages) or all
 *     on one device of the context (used in place); anything else is ZC_ERR_MIXED_MEM.  Device arrays need 8-byte alignment
 *     only.
 *   - The call writes the 32 bytes of out32 and rows 0 .. n-1 of ok, nothing else, and no byte of any input.  It runs on
 *     the context's stream and shares the MSM workspace of its device slot with zc_msm. */
int zc_ris_lincomb_sum(zc_ctx *ctx, const uint8_t *in32, const uint64_t *scalars, size_t terms,
                       const uint64_t *base_scalars, const uint64_t *weights,
                       uint8_t *out32, uint8_t *ok, size_t n);

#ifdef __cplusplus
}
#endif

#endif /* ZEROCAF_HIP_EXT_SUM_H */
