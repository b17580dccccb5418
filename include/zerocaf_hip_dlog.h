/*
 * zerocaf_hip_dlog.h -- additive entry points beyond the 0.6 table: BOUNDED DISCRETE LOGS, m_i with P_i = m_i * G and
 * 0 <= m_i < bound, by baby steps from a table and giant steps per row.
 *
 * A header of its own: a caller includes it beside zerocaf_hip.h (it is not a part of zerocaf_hip_ext.h).  Same libraries and
 * conventions as everything in zerocaf_hip.h (status codes, host or device arrays, the context's stream); zc_version() stays as
 * it is.  Plain C11.
 */
#ifndef ZEROCAF_HIP_DLOG_H
#define ZEROCAF_HIP_DLOG_H

#include "zerocaf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Exponential ElGamal under one key (zc_ed_scalar_mul_shared, zc_ris_mul_shared), its decryption as the pair (1, -x)
 * (zc_ed_lincomb_shared, zc_ris_lincomb_shared) and its tally (zc_ed_sum_rows, zc_ris_sum_rows) all end in a batch of points
 * M_i = m_i * G with small m_i: a vote count, an amount, a share index.  These calls recover m_i.  The same step opens a Pedersen
 * commitment whose blinding is known and turns key images back into indices.
 *
 * zc_dlog_create: point is 20 limbs, in host memory or on a device of the context.  X, Y and Z are read; T is ignored.
 *   G_eff = G without flags, 4 * G with ZC_DLOG_COSET4.  The call builds, synchronously and on EVERY device slot of the context,
 *     - the baby-step table: the records of j * G_eff, 0 <= j < 2^table_bits, 32 bytes each (an internal fingerprint of the affine
 *       point: canonical y, the parity of canonical x in bit 255; injective on curve points with Z != 0), and 2^(table_bits + 1)
 *       hash slots of 8 bytes over them: 48 * 2^table_bits bytes, 192 MB at table_bits = 22;
 *     - the stride point -2^table_bits * G_eff;
 *     - 64 launch offsets (below).
 *   The records are computed on the device, the hash slots filled on the host in index order: their layout depends on the
 *   records only.  When the call returns, point may be overwritten or freed.
 *   - ZC_ERR_BAD_ARG in this order: "null pointer: point", "null pointer: id_out", "zc_dlog_create: table_bits must be
 *     ZC_DLOG_MIN_BITS .. ZC_DLOG_MAX_BITS", "zc_dlog_create: unknown flag bits", "null context", "zc_dlog_create: not a point of
 *     the curve" (the rule of zc_gens_create: the curve equation and Z != 0 mod p BY VALUE -- the limbs of p, 2p ... are zero too),
 *     "zc_dlog_create: generator lies in E[8]" when 8 * G_eff is the identity.  Nothing is created and *id_out is not written.
 *     point on a device outside the context is ZC_ERR_MIXED_MEM.
 *   WHY AT MOST ONE m MATCHES.  The curve group has order 8 L with L prime, so the order of a point divides 8 L.  If 8 * G_eff is
 *   not the identity that order does not divide 8, hence is a multiple of L > 2^249.  Two multiples m * G_eff and m' * G_eff with
 *   0 <= m, m' < 2^38 are then different points unless m = m': no two table entries coincide, and at most one m below
 *   2^table_bits * ZC_DLOG_MAX_STEPS <= 2^38 matches a row.  (The host refuses a table in which a record occurs twice all the
 *   same, "zc_dlog_create: two table entries coincide": a backstop that cannot trigger.)
 *   *id_out: nonzero, drawn from the same process-wide counter as the ids of zc_msm_bases_create and zc_gens_create -- an id of
 *   one kind is never valid for another -- and never reused.
 *
 * zc_dlog_destroy: waits for the streams of every device slot of the context, then frees the table.  zc_ctx_destroy frees every
 *   live table.  An unknown, destroyed or foreign id -- an id of zc_msm_bases_create or zc_gens_create included -- is
 *   ZC_ERR_BAD_ARG, "unknown dlog table"; the two row calls answer such an id in the same way.
 *
 * zc_ed_dlog: p is n * 20 limbs.  found[i] = 1 and m_out[i] = m iff there is an m with 0 <= m < bound and P_i == m * G as Edwards
 *   points (zc_ed_eq); with a ZC_DLOG_COSET4 table iff 4 * P_i == m * (4 * G), that is P_i - m * G in E[4]: Ristretto equality.
 *   Otherwise found[i] = 0 and m_out[i] = 0.  bound is exact: it need not be a multiple of the table size, and a match with
 *   m >= bound inside the last giant step is NOT reported.  1 <= bound <= 2^table_bits * ZC_DLOG_MAX_STEPS, else ZC_ERR_BAD_ARG,
 *   "<name>: bound must be 1 .. 2^table_bits * ZC_DLOG_MAX_STEPS".
 *   ok may be NULL.  ok[i] = 0 for a row that is no point of the curve or has Z = 0 mod p by value; such a row gets found[i] = 0,
 *   m_out[i] = 0 and changes no other row (a row's shared inversion lives inside its own lane).  T of a row is not read.
 *   The answer does not depend on the projective representative, the batch size, the memory placement or the launch form.
 *   Cost: a row walks Q_g = P_i - g * 2^table_bits * G_eff for g = 0, 1, ... and stops at its match: about 11 field
 *   multiplications per giant step plus a quarter of an inversion, ceil(bound / 2^table_bits) steps for a row without a match;
 *   the rows of a wave leave together, when the last of them is through.
 *   No launch runs more than 1024 giant steps: launch k starts from Q_0 + W_k, W_k = -k * 1024 * 2^table_bits * G_eff from the
 *   table's 64 offsets, skips rows that are found and leaves the others as they are; launch 0 writes the not-found defaults.
 *   All launches go on the context's stream.
 *
 * zc_ris_dlog: in32 is n * 32 bytes, Ristretto encodings; the row's point is its decoding.  The call needs a ZC_DLOG_COSET4
 *   table: otherwise ZC_ERR_BAD_ARG, "zc_ris_dlog needs a ZC_DLOG_COSET4 table".  A row that does not decode gets ok[i] = 0,
 *   found[i] = 0, m_out[i] = 0.  32 zero bytes are the identity: m = 0.
 *
 *   - ZC_ERR_BAD_ARG before n == 0 and before the context is looked at, in this order: "null pointer: p" / "null pointer: in32",
 *     "null pointer: m_out", "null pointer: found", "null context", the id ("unknown dlog table"), the COSET4 rule of
 *     zc_ris_dlog, the bound, then n >= 2^31 ("<name>: n must stay below 2^31").
 *   - n == 0: ZC_OK, nothing written.
 *   - All arrays in host memory (staged in chunks, synchronous, sharded over the devices of a multi-device context) or all on
 *     one device of the context (used in place, asynchronous on the context's stream); anything else is ZC_ERR_MIXED_MEM.
 *     Device arrays of limbs and of m_out need 8-byte alignment only.
 *   - The calls write rows 0 .. n-1 of m_out, found and ok and nothing else.
 *   - No environment knob.
 *   - Nothing in this library is constant-time: the giant steps a row walks, the slots and the records it reads depend on m.
 *   - A table must outlive the calls that use it: destroy it from the thread that issues them, or after they have returned. */
#define ZC_DLOG_MIN_BITS 4
#define ZC_DLOG_MAX_BITS 22
#define ZC_DLOG_MAX_STEPS 65536          /* giant steps per call */
#define ZC_DLOG_COSET4 1u                /* flags: equality modulo E[4] -- Ristretto equality */
int zc_dlog_create(zc_ctx *ctx, const uint64_t *point, unsigned table_bits, unsigned flags, uint64_t *id_out);
int zc_dlog_destroy(zc_ctx *ctx, uint64_t id);
int zc_ed_dlog(zc_ctx *ctx, uint64_t id, const uint64_t *p, uint64_t bound, uint64_t *m_out, uint8_t *found, uint8_t *ok, size_t n);
int zc_ris_dlog(zc_ctx *ctx, uint64_t id, const uint8_t *in32, uint64_t bound, uint64_t *m_out, uint8_t *found, uint8_t *ok, size_t n);

#ifdef __cplusplus
}
#endif

#endif /* ZEROCAF_HIP_DLOG_H */
