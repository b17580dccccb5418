/*
 * zerocaf_hip_ext_shared_lincomb.h -- additive entry points beyond the 0.6 table: ONE scalar VECTOR applied to a whole batch,
 * out[i] = k_0 * P_i0 + k_1 * P_i1 + ... with the same coefficients in every row.
 *
 * Part of zerocaf_hip_ext.h, which includes this file after zerocaf_hip_ext_shared.h: a caller includes that header (or this one
 * alone) and finds the declarations below.  Same libraries and conventions as everything in zerocaf_hip.h (status codes, host or
 * device arrays, the context's stream); zc_version() stays as it is.  Plain C11.
 */
#ifndef ZEROCAF_HIP_EXT_SHARED_LINCOMB_H
#define ZEROCAF_HIP_EXT_SHARED_LINCOMB_H

#include "zerocaf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The shared-scalar protocols rarely stop at k * P_i: ElGamal decryption under one key is M_i = C2_i - x * C1_i, coefficients
 * (1, -x mod L); threshold decryption combines the shares D_ij with Lagrange coefficients that are the same for every
 * ciphertext; the generator folding of an inner-product argument is G'_i = u^-1 * G_i + u * G_(i + n/2).  These calls are
 * zc_ed_lincomb and zc_ris_lincomb for such a batch: one doubling chain per row, one addition per non-zero window digit of any
 * term, a coefficient 1 that costs one table record, a coefficient 0 that costs nothing.
 *
 * points: n * terms * 20 limbs, row-major like zc_ed_lincomb (the terms of row i are consecutive).  in32: n * terms * 32 bytes,
 * row-major like zc_ris_lincomb.  terms is 1 .. ZC_LINCOMB_MAX_TERMS, and n * terms stays below 2^31.
 *
 * k is ONE scalar vector: terms * 5 words, radix 2^52, ALWAYS HOST memory.  The call reads and recodes it before it returns:
 * the caller may overwrite k as soon as the call returns, also when the row arrays are on the device and the work is still in
 * flight.  A device pointer for k is ZC_ERR_BAD_ARG ("k must be host memory").  Each k_j is read exactly as
 * zc_ed_scalar_mul_shared reads its scalar: limb bits from 2^52 up are masked, and a pattern of 2^256 or more follows the
 * reference's early-stop rule.  The library keeps no copy of k or of its digits after the launches it issued.
 *
 * The schedule of doublings and additions -- and therefore the running time -- DEPENDS ON k.  Nothing in this library is
 * constant-time.
 *
 * zc_ed_lincomb_shared: out[i] = the same group element as the reference's ((k_0 * P_i0 + k_1 * P_i1) + ...), Mul<Scalar> and
 *   Add in index order, under the contract of ZC_SCALAR_MUL_FAST: equal under == (zc_ed_eq), identical encodings, limbs that
 *   are deterministic and the same in every launch form, batch size and memory placement -- but another projective
 *   representative than the reference's.  Torsion and mixed-order points are multiplied by the integer k_j, not by k_j mod L.
 *   A row that holds a point off the curve gets deterministic garbage for its own row only: unlike zc_ed_lincomb there is
 *   no second strict pass.  out must not overlap points unless terms == 1; for terms == 1 out may be exactly points, and the
 *   limbs are those of zc_ed_scalar_mul_shared.
 *
 * zc_ris_lincomb_shared: out32[i] = compress(sum_j k_j * decompress(in32[i][j])), byte-identical to zc_ris_lincomb with
 *   base_scalars = NULL and the same terms scalars in every row.  A row with an undecodable term gets 32 zero bytes and
 *   ok = 0 whatever the scalars -- a zero scalar on that term does not change this.  A row whose sum is the identity gets 32
 *   zero bytes and ok = 1.  ok may be NULL.  The call ignores ZC_RISTRETTO_STRICT.  It walks (k_j mod L) / 2 mod L and encodes
 *   the double of the sum, which needs one shared-formula inversion and no square root.  For terms == 1 the bytes are those of
 *   zc_ris_mul_shared.  There is NO basepoint term: a caller who needs one passes the encoding of B as a term.
 *
 *   - ZC_ERR_BAD_ARG before n == 0 and before the context, in this order: "null pointer: points" / "null pointer: in32", "null
 *     pointer: k", "null pointer: out" / "null pointer: out32"; terms outside 1 .. ZC_LINCOMB_MAX_TERMS; n * terms >= 2^31; then
 *     the context ("null context").
 *   - n == 0: ZC_OK, nothing written.
 *   - The row arrays all in host memory (staged in chunks, synchronous, sharded over the devices of a multi-device context) or
 *     all on one device of the context (used in place, asynchronous on the context's stream); anything else is
 *     ZC_ERR_MIXED_MEM.  Device arrays need 8-byte alignment only.
 *   - The call writes rows 0 .. n-1 of its outputs and nothing else.
 *   - No environment knob. */
int zc_ed_lincomb_shared(zc_ctx *ctx, const uint64_t *points, const uint64_t *k, size_t terms, uint64_t *out, size_t n);
int zc_ris_lincomb_shared(zc_ctx *ctx, const uint8_t *in32, const uint64_t *k, size_t terms, uint8_t *out32, uint8_t *ok, size_t n);

#ifdef __cplusplus
}
#endif

#endif /* ZEROCAF_HIP_EXT_SHARED_LINCOMB_H */
