/*
 * zerocaf_hip_ext_gens.h -- additive entry points beyond the 0.6 table: GENERATOR SETS, a few fixed points of the caller's and
 * one scalar per point and row, out[i] = k_i0 * G_0 + k_i1 * G_1 + ...
 *
 * Part of zerocaf_hip_ext.h, which includes this file after zerocaf_hip_ext_shared_lincomb.h: a caller includes that header (or
 * this one alone) and finds the declarations below.  Same libraries and conventions as everything in zerocaf_hip.h (status
 * codes, host or device arrays, the context's stream); zc_version() stays as it is.  Plain C11.
 */
#ifndef ZEROCAF_HIP_EXT_GENS_H
#define ZEROCAF_HIP_EXT_GENS_H

#include "zerocaf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* zc_ed_mul_base and zc_ris_mul_base_compress multiply the curve basepoint from a comb table: 33 mixed additions per scalar,
 * no doublings.  Protocols have other fixed points: the second Pedersen generator H of v * G + r * H, a recipient key PK of an
 * ElGamal encryption (r * B, M + r * PK), the two bases of a DLEQ prover, per-asset generators.  A generator set holds such
 * points with a comb table each, and the two row calls are the basepoint calls over it: 33 mixed additions per term against
 * the 1827 + 567 * terms multiplications of zc_ed_lincomb with the same points tiled into every row.
 *
 * zc_gens_create: points is count * 20 limbs, count = 1 .. ZC_GENS_MAX, in host memory or on a device of the context.  Only X, Y
 *   and Z of a point are read; T is ignored.  Each generator is normalised to Z = 1 and its table T_j[w][e] = (e + 1) * 256^w *
 *   G_j is built on the device: 33 x 128 cached affine records of 128 bytes, about 540 KB per generator, on EVERY device slot
 *   of the context (host batches are sharded as for every other row-wise call).  The call is synchronous: when it returns the
 *   tables are complete and visible to any stream, and points may be overwritten or freed.
 *   A generator must satisfy the curve equation with Z != 0 mod p BY VALUE (ZERO IS DECIDED BY VALUE, zerocaf_hip.h: the limbs
 *   of p, 2p ... are zero too).  Otherwise the call returns ZC_ERR_BAD_ARG, "zc_gens_create: generator %d is not a point of the
 *   curve" with the index of the first such generator; nothing is created and *id_out is not written.  The check runs on the
 *   device.  Torsion and mixed-order points, the identity and repeated or mutually negated generators are all legal.
 *   *id_out: nonzero, drawn from the same process-wide counter as the ids of zc_msm_bases_create -- an id of one kind is never
 *   valid for the other -- and never reused.
 *   - ZC_ERR_BAD_ARG in this order: "null pointer: points", "null pointer: id_out", "zc_gens_create: count must be 1 ..
 *     ZC_GENS_MAX", "null context"; points on a device outside the context is ZC_ERR_MIXED_MEM.
 *
 * zc_gens_destroy: waits for the streams of every device slot of the context, then frees the tables.  zc_ctx_destroy frees
 *   every live set.  An unknown, destroyed or foreign id -- an id of zc_msm_bases_create included -- is ZC_ERR_BAD_ARG,
 *   "unknown generator set"; the two row calls answer such an id in the same way.
 *
 * scalars: n * count * 5 limbs, row-major (the count scalars of row i are consecutive).  Each scalar is read exactly as
 * zc_ed_mul_base reads its scalar: raw limbs, bits from 2^52 up ignored, and a pattern of 2^256 or more follows the
 * reference's early-stop rule.
 *
 * zc_ed_mul_gens: out[i] = sum_j scalars[i][j] * G_j, n x 20 limbs: the same group element as the reference's ((k_0 * G_0 + k_1 *
 *   G_1) + ...), Mul<Scalar> and Add in index order, under the contract of ZC_SCALAR_MUL_FAST: equal under == (zc_ed_eq),
 *   identical encodings, limbs that are deterministic and the same in every launch form, batch size and memory placement --
 *   but another projective representative than the reference's.  Points are multiplied by the integer k, not by k mod L.
 *
 * zc_ris_mul_gens_compress: out32[i] = compress of that sum, n x 32 bytes, identical to zc_ris_compress of zc_ed_mul_gens's
 *   output and to the reference's composition.  An identity sum gives 32 zero bytes.  There is no ok output: nothing is
 *   decoded.
 *
 *   - ZC_ERR_BAD_ARG before n == 0 and before the context is looked at, in this order: "null pointer: scalars", "null pointer:
 *     out" / "null pointer: out32", "null context", the id ("unknown generator set"), then n * count >= 2^31 ("<name>: n * count
 *     must stay below 2^31").
 *   - n == 0: ZC_OK, nothing written.
 *   - Both arrays in host memory (staged in chunks, synchronous, sharded over the devices of a multi-device context) or both
 *     on one device of the context (used in place, asynchronous on the context's stream); anything else is
 *     ZC_ERR_MIXED_MEM.  Device arrays need 8-byte alignment only.
 *   - The calls write rows 0 .. n-1 of their output and nothing else.
 *   - No environment knob.
 *   - Nothing in this library is constant-time: the additions a wave makes and the table records it reads depend on the
 *     scalars.
 *   - A set must outlive the calls that use it: destroy it from the thread that issues them, or after they have returned. */
#define ZC_GENS_MAX 8
int zc_gens_create(zc_ctx *ctx, const uint64_t *points, size_t count, uint64_t *id_out);
int zc_gens_destroy(zc_ctx *ctx, uint64_t id);
int zc_ed_mul_gens(zc_ctx *ctx, uint64_t id, const uint64_t *scalars, uint64_t *out, size_t n);
int zc_ris_mul_gens_compress(zc_ctx *ctx, uint64_t id, const uint64_t *scalars, uint8_t *out32, size_t n);

#ifdef __cplusplus
}
#endif

#endif /* ZEROCAF_HIP_EXT_GENS_H */
