/*
 * zerocaf_hip_scvec.h -- additive entry points beyond the 0.6 table: SCALAR VECTOR OPS mod L, the reductions and the power rows
 * the element-wise scalar calls (zc_sc_add, zc_sc_mul, zc_sc_muladd, ...) leave out: out[i] = sum_j a_ij, out[i] = sum_j a_ij b_ij
 * and out[i][j] = x_i^j.
 *
 * A header of its own: a caller includes it beside zerocaf_hip.h (it is not a part of zerocaf_hip_ext.h).  Same libraries and
 * conventions as everything in zerocaf_hip.h (status codes, host or device arrays, the context's stream); zc_version() stays as
 * it is.  Plain C11.
 */
#ifndef ZEROCAF_HIP_SCVEC_H
#define ZEROCAF_HIP_SCVEC_H

#include "zerocaf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* An inner-product argument needs <a, b>, <a, y^n> and the row y^0 .. y^(n-1); a range-proof verifier the rows z^2 * 2^j; a
 * batch verifier that keeps its own b = sum z_i * s_i a weighted sum; a Shamir dealer evaluates a polynomial (a dot product with
 * a power row); a tally may weight its ballots.  These calls keep all of that on the device, the rows read once.
 *
 * Values.  Everything is BY VALUE, exactly as zerocaf_hip.h states it for zc_sc_muladd: val(w) = sum (w_i mod 2^52) 2^(52 i) for
 *   the five words of a scalar; bits at or above 2^52 of a word are ignored, so a value has up to 260 bits and need not be
 *   reduced.  Every output is the canonical five limbs of the stated residue mod L.
 *
 * zc_sc_sum_rows: a is n * terms * 5 limbs, row-major like zc_ed_sum_rows: row i owns the `terms` consecutive records
 *   a[(i * terms + j) * 5 ..].  out[i], n x 5 limbs, is sum_j val(a[i][j]) mod L.
 *
 * zc_sc_dot_rows: out[i] = sum_j val(a[i][j]) * val(b[i][j]) mod L; b has the shape of a.  With flags = ZC_SC_DOT_SHARED_B, b is
 *   ONE row of terms * 5 limbs that every row uses -- weights, Lagrange coefficients, a challenge vector, y^n; it is read through
 *   the cache, not n times from memory, and from host memory it goes to each device once.  Any other flag bit is
 *   ZC_ERR_BAD_ARG, "zc_sc_dot_rows: unknown flag bits".
 *
 * zc_sc_powers: x is n * 5 limbs, out is n * terms * 5 limbs: out[i][j] = val(x_i)^j mod L for 0 <= j < terms.  out[i][0] = 1 also
 *   for an x that is 0 mod L.  A polynomial evaluation is zc_sc_dot_rows of the coefficients with such a row.
 *
 * terms is any value >= 0; it is not capped at 8.  Both shapes are meant: millions of short rows, and one row of 2^24 terms
 *   (n = 1).  terms == 0 gives zero rows for the sum and the dot product; zc_sc_powers then writes nothing.
 *
 * Addition mod L is associative and every result is canonical: the outputs depend on the row's values alone, not on n, on the rows
 *   beside it, on the memory placement or on the launch form.
 *
 *   - ZC_ERR_BAD_ARG before n == 0, by name and in this order: "null pointer: a" (zc_sc_powers: "null pointer: x"),
 *     "null pointer: b", "null pointer: out", the unknown flag bits, "null context", then n * terms >= 2^31
 *     ("<name>: n * terms must stay below 2^31").
 *   - n == 0: ZC_OK, nothing written.
 *   - All arrays in host memory (staged in chunks of whole rows, synchronous, the rows sharded over the devices of a multi-device
 *     context; a row longer than a staging chunk goes up through the staging buffers into device memory the call sizes for it,
 *     as in zc_ed_sum_rows) or all on one device of the context (used in place, asynchronous on the context's stream);
 *     anything else is ZC_ERR_MIXED_MEM.  Device arrays need 8-byte alignment only.
 *   - Outputs must not overlap inputs.
 *   - The calls write rows 0 .. n-1 of out and nothing else; no row changes another row's result.
 *   - Sums and dot products of rows of more than 32768 terms keep their partial sums in a workspace of the context's device slot
 *     between two kernels; calls in flight on different streams are ordered as for every other call of the context.
 *   - No environment knob.
 *   - Nothing in this library is constant-time. */
#define ZC_SC_DOT_SHARED_B 1u            /* flags: b is one row of terms * 5 limbs for every row */
int zc_sc_sum_rows(zc_ctx *ctx, const uint64_t *a, size_t terms, uint64_t *out, size_t n);
int zc_sc_dot_rows(zc_ctx *ctx, const uint64_t *a, const uint64_t *b, size_t terms, unsigned flags, uint64_t *out, size_t n);
int zc_sc_powers  (zc_ctx *ctx, const uint64_t *x, size_t terms, uint64_t *out, size_t n);

#ifdef __cplusplus
}
#endif

#endif /* ZEROCAF_HIP_SCVEC_H */
