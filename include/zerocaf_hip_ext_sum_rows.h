/*
 * zerocaf_hip_ext_sum_rows.h -- additive entry points beyond the 0.6 table: POINT SUMS, the plain group operation over rows of
 * any length, out[i] = P_i0 + P_i1 + ... + P_i(terms-1), on points and on Ristretto encodings.
 *
 * Part of zerocaf_hip_ext.h, which includes this file after zerocaf_hip_ext_gens.h: a caller includes that header (or this one
 * alone) and finds the declarations below.  Same libraries and conventions as everything in zerocaf_hip.h (status codes, host
 * or device arrays, the context's stream); zc_version() stays as it is.  Plain C11.
 */
#ifndef ZEROCAF_HIP_EXT_SUM_ROWS_H
#define ZEROCAF_HIP_EXT_SUM_ROWS_H

#include "zerocaf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* zc_ed_add adds one pair per row; zc_msm, zc_ed_lincomb and zc_ed_mul_gens sum scalar multiples.  These two calls are the
 * reduction between them: an ElGamal tally over many ballots, an aggregate of public keys or commitments, a balance check
 * sum(inputs) - sum(outputs), the fold of partial results of any kind.  One addition (9 field multiplications) per point, the
 * row read once.
 *
 * points: n * terms * 20 limbs, row-major: row i owns the `terms` consecutive records points[(i * terms + j) * 20 ..], as in
 *   zc_ed_lincomb.  in32: n * terms * 32 bytes, likewise.  terms is any value >= 0; it is not capped at 8.  Both shapes are meant:
 *   millions of short rows, and one row of 2^24 points (n = 1).  A point is read exactly as zc_ed_add reads one: all 20 limbs,
 *   any 52-bit limb pattern standing for its value mod p.  Ragged rows: pad with identity points (0, 1, 1, 0), in the wire form
 *   with 32 zero bytes.
 *
 * zc_ed_sum_rows: out[i], n x 20 limbs, is the sum of row i under the reference's unified addition (src/edwards.rs:465-489) in an
 *   ORDER OF ASSOCIATION THAT IS A FUNCTION OF terms ALONE:
 *     1. P = parts(terms), a power of two:  P = 1 for terms <= 32; otherwise the largest power of two with 16 * P <= terms,
 *        at most 2^16.
 *     2. Slice s (0 <= s < P) holds the points s, s + P, s + 2 P, ... of the row.
 *     3. Each slice is folded from the left in index order, starting from its first point.
 *     4. The P partial sums q_0 .. q_(P-1) are combined by adjacent pairs, q'_s = q_(2s) + q_(2s+1), level by level, until one
 *        is left.
 *   With P = 1 this is the plain left fold ((P_0 + P_1) + P_2) + ..., limb for limb what zc_ed_fold_ordered returns.  The output
 *   limbs are canonical and a function of the row's points and of terms: they do not depend on n, on the rows beside it, on the
 *   memory placement or on the launch form, and they are the limbs of the reference's addition applied in that order.
 *   A row of one term is its point with every coordinate reduced mod p (as zc_ed_fold_ordered returns a list of one).
 *   terms == 0 gives identity rows (0, 1, 1, 0).  A record that is no curve point gives deterministic garbage for its own row.
 *
 * zc_ris_sum_rows: out32[i] = compress(sum_j decompress(in32[i][j])), n x 32 bytes, with the reference's decompress and
 *   compress; the bytes are those of that composition in any order of association, since an encoding depends on the group
 *   element only.  A row with an undecodable term gets ok[i] = 0 and 32 zero bytes; every other row gets ok[i] = 1, and an
 *   identity sum is 32 zero bytes with ok = 1.  ok may be NULL.  terms == 0 gives 32 zero bytes with ok = 1.  No intermediate
 *   point reaches the caller's memory.
 *
 *   - ZC_ERR_BAD_ARG before n == 0, in this order: "null pointer: points" / "null pointer: in32", "null pointer: out" /
 *     "null pointer: out32", "null context", then n * terms >= 2^31 ("<name>: n * terms must stay below 2^31").
 *   - n == 0: ZC_OK, nothing written.
 *   - All non-NULL arrays in host memory (staged in chunks of whole rows, synchronous, the rows sharded over the devices of a
 *     multi-device context; a row longer than a staging chunk goes up through the staging buffers into device memory the call
 *     sizes for it and is summed there) or all on one device of the context (used in place, asynchronous on the context's
 *     stream); anything else is ZC_ERR_MIXED_MEM.  Device arrays need 8-byte alignment only.
 *   - Outputs must not overlap inputs.
 *   - The calls write rows 0 .. n-1 of out / out32 / ok and nothing else; no row changes another row's result.
 *   - Rows of more than 8191 terms keep their partial sums in a workspace of the context's device slot between two kernels;
 *     calls in flight on different streams are ordered as for every other call of the context.
 *   - No environment knob.
 *   - Nothing in this library is constant-time. */
int zc_ed_sum_rows (zc_ctx *ctx, const uint64_t *points, size_t terms, uint64_t *out, size_t n);
int zc_ris_sum_rows(zc_ctx *ctx, const uint8_t *in32, size_t terms, uint8_t *out32, uint8_t *ok, size_t n);

#ifdef __cplusplus
}
#endif

#endif /* ZEROCAF_HIP_EXT_SUM_ROWS_H */
