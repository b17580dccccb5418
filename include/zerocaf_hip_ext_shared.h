/*
 * zerocaf_hip_ext_shared.h -- additive entry points beyond the 0.6 table: ONE scalar applied to a whole batch of points.
 *
 * Part of zerocaf_hip_ext.h, which includes this file: a caller includes that header (or this one alone) and finds the
 * declarations below.  Same libraries and conventions as everything in zerocaf_hip.h (status codes, host or device arrays, the
 * context's stream); zc_version() stays as it is.  Plain C11.
 */
#ifndef ZEROCAF_HIP_EXT_SHARED_H
#define ZEROCAF_HIP_EXT_SHARED_H

#include "zerocaf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The transpose of zc_msm_fixed: one secret scalar, many points -- a view-key scan (a * R_i for every output R_i), an OPRF or
 * PSI server (k * P_i for every client point), ElGamal decryption or re-randomisation under one key.
 *
 * The scalar k is ONE scalar: five words, radix 2^52, ALWAYS HOST memory.  The call reads and recodes it before it returns:
 * the caller may overwrite k as soon as the call returns, also when the row arrays are on the device and the work is still in
 * flight.  A device pointer for k is ZC_ERR_BAD_ARG ("k must be host memory").  The value multiplied by is the one
 * double_and_add multiplies by -- limb bits from 2^52 up are masked, and a pattern of 2^256 or more follows the reference's
 * early-stop rule -- exactly as zc_ed_scalar_mul and zc_ris_roundtrip_mul read the same five words in every row.  The
 * library keeps no copy of k or of its digits after the launches it issued.
 *
 * The schedule of doublings and additions -- and therefore the running time -- DEPENDS ON k (its length and its non-zero
 * digits).  That is no different from every other call here: nothing in this library is constant-time.
 *
 * zc_ed_scalar_mul_shared: out[i] = k * P_i, the same group element as the reference's Mul<Scalar> (src/edwards.rs:104-126), under
 *   the contract of ZC_SCALAR_MUL_FAST: equal under == (zc_ed_eq), identical encodings, limbs that are deterministic and the
 *   same in every launch form, batch size and memory placement -- but another projective representative than the
 *   reference's.  Torsion and mixed-order points are multiplied by the integer, not by k mod L.  A row that is no curve point
 *   gets deterministic garbage for its own row only.  out may be exactly p.
 *
 * zc_ris_mul_shared: out32[i] = compress(k * decompress(in32[i])), byte-identical to zc_ris_roundtrip_mul with k in every
 *   row.  An undecodable row gets 32 zero bytes and ok = 0; a decodable row whose product is the identity gets 32 zero bytes
 *   and ok = 1.  ok may be NULL.  out32 may be exactly in32.  The call ignores ZC_RISTRETTO_STRICT.  It multiplies by
 *   (k mod L) / 2 mod L and encodes the double of the result, which needs one shared-formula inversion and no square root.
 *
 *   - ZC_ERR_BAD_ARG before n == 0 and before the context, in this order: "null pointer: p" / "null pointer: in32", "null
 *     pointer: k", "null pointer: out" / "null pointer: out32"; then the context ("null context").
 *   - n == 0: ZC_OK, nothing written.
 *   - The row arrays all in host memory (staged in chunks, synchronous, sharded over the devices of a multi-device context) or
 *     all on one device of the context (used in place, asynchronous on the context's stream); anything else is
 *     ZC_ERR_MIXED_MEM.  Device arrays need 8-byte alignment only.
 *   - The call writes rows 0 .. n-1 of its outputs and nothing else.
 *   - No environment knob. */
int zc_ed_scalar_mul_shared(zc_ctx *ctx, const uint64_t *p, const uint64_t *k, uint64_t *out, size_t n);
int zc_ris_mul_shared(zc_ctx *ctx, const uint8_t *in32, const uint64_t *k, uint8_t *out32, uint8_t *ok, size_t n);

#ifdef __cplusplus
}
#endif

#endif /* ZEROCAF_HIP_EXT_SHARED_H */
