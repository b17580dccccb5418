// zc_scvec.hip.h -- scalar vector ops mod L (zerocaf_hip_scvec.h): out[i] = sum_j a_ij, out[i] = sum_j a_ij b_ij and
// out[i][j] = x_i^j over rows of any length.  Everything is by value: val(w) = sum (w_i mod 2^52) 2^(52 i), any 260-bit pattern, and
// every output is the canonical residue; addition mod L is associative, so the cut of a row (zc_scvec_plan.h) changes no result.
//
// Sums and dot products: lane t of a workgroup is (row t / W, slice t % W) of its W = min(P, 256) slices.  Every byte comes in
// through LDS with 8-byte loads that run along the addresses.  Rows of up to 1024 terms: P = 1 .. 256 with at most four records per
// lane, so that the rows of a workgroup are one contiguous block of at most 1024 records, staged whole; a lane picks its records
// out of LDS.  Longer rows: one row per workgroup (or 256 slices of it), at every fold step neighbouring lanes want neighbouring
// 40-byte records, two steps staged at a time as in zc_sum.hip.h.  The same LDS then holds the partials of the tree.
//   dot product   81 multiply-adds per term into 17 unreduced 64-bit columns, a carry pass (17 shifts) every 7 products, and ONE
//                 reduction per slice: Montgomery reduction of the 18 limbs (54), the nineteenth limb brought in when the slice
//                 has more than 4 products (135), one multiplication by R^2 (135).  A chain of sc_muladd_limbs52 is 151 per term.
//   sum           nine 64-bit adds per term (a column takes 2^31 limbs of 29 bits), the same reduction per slice.
//   tree          canonical partials: add, carry, one conditional subtraction per pair.
// Powers: lane l of a group of G lanes holds x^l and x^G from one square-and-multiply over the bits of l and writes
// x^l, x^(l + G), ...: one Montgomery multiplication and one reduction to canonical form per record (135 + 54), records staged in
// LDS and written out in address order.
#pragma once
#include "zc_arith.hip.h"
#include "zc_scvec_plan.h"

namespace zc {

// The 17 columns of sum a b in radix 2^29, column 17 for what a carry pass pushes beyond them.
struct scv_cols {
    u64 t[18];
};
ZC_DI void scv_cols_zero(scv_cols& c)
{
#pragma unroll
    for (int k = 0; k < 18; k++) c.t[k] = 0;
}
// Columns 0..16 back below 2^29; column 17 keeps everything above 2^493 (m products: below m 2^27).
ZC_DI void scv_cols_carry(scv_cols& c)
{
#pragma unroll
    for (int k = 0; k < 17; k++) {
        c.t[k + 1] += c.t[k] >> 29;
        c.t[k] &= M29;
    }
}
// c += a b for normalized limbs (limb 8 below 2^29): a column grows by less than 9 * 2^58.
ZC_DI void scv_cols_mac(scv_cols& c, const fe& a, const fe& b)
{
    for (int k = 0; k < 17; k++) ZC_ASSERT(c.t[k] <= ~0ull - (9ull << 58));               // room for one more product
#pragma unroll
    for (int i = 0; i < 9; i++)
#pragma unroll
        for (int j = 0; j < 9; j++) c.t[i + j] += (u64)a.v[i] * b.v[j];
}
// The columns' value X mod L, canonical.  After the carry pass X = LO + hi 2^522 with LO of eighteen 29-bit limbs and hi < 2^29
// (X < 2^551: any slice below 2^31 products of 260-bit values).  Montgomery reduction leaves LO / R below 2^261 + L (R = 2^261);
// hi 2^522 / R = hi R is the Montgomery product of hi and R^2, below 3 L; the lazy sum times R^2 over R is X mod L below 3 L
// ((2^261 + 4 L) L / R + L), and two conditional subtractions make it canonical.  nohi: the caller knows X < 2^522.
ZC_DI fe scv_cols_fold(scv_cols& c, bool nohi)
{
    typedef ModL F;
    scv_cols_carry(c);
    const u64 top = c.t[17];
    ZC_ASSERT((top >> 58) == 0);                                                         // hi < 2^29
    ZC_ASSERT(!nohi || (top >> 29) == 0);
    c.t[17] = top & M29;
    fe r;
    mont_reduce_cols<F>(r, c.t);
    ZC_ASSERT(r.v[8] <= (1u << 29) + (1u << F::TOPSHIFT));                                // LO / R < 2^261 + L
    if (!nohi) {
        fe h = fe_zero();
        h.v[0] = (u32)(top >> 29);
        r = fe_add(r, mont_mul<F>(h, fe_const<F>(F::RR)));
    }
    return fe_cond_sub_n<F>(fe_cond_sub_n<F>(mont_mul<F>(r, fe_const<F>(F::RR))));
}
// a + b mod L for canonical a, b
ZC_DI fe scv_pair(const fe& a, const fe& b)
{
    fe r = fe_add(a, b);
    fe_carry(r);
    return fe_cond_sub_n<ModL>(r);
}

// Fold steps every lane of a launch walks through: the longest slice's (slice 0), ceil(terms / parts).
ZC_DI u32 scv_fold_steps(u32 terms, u32 parts) { return (terms + parts - 1) / parts; }
// Where record j of row `row` lies in b, in records: a shared b is one row that every row uses.
ZC_DI size_t scv_b_record(bool shared_b, size_t row, size_t terms, size_t j) { return (shared_b ? 0 : row * terms) + j; }

// Slice s of a row of `terms` records cut into `parts`: the records s, s + parts, ...  load(k, j, have, xa[, xb]) brings record j of
// the row in step k; it is called in every one of the `steps` steps, also past the slice's end (have false: the staged loader of
// the kernels has barriers inside, and every lane of a workgroup walks the same steps).  A lane without a row passes terms = 0.
#ifndef ZC_SCV_DOT_CHAINED
#define ZC_SCV_DOT_CHAINED 0      // 1: A/B build on a chain of sc_muladd_limbs52, 151 multiply-adds per term (tools/bench_scvec.py --ab-lib)
#endif
template <class LOAD>
ZC_DI fe scv_slice_dot(size_t terms, size_t parts, size_t s, size_t steps, LOAD&& load)
{
#if ZC_SCV_DOT_CHAINED
    u64 r[5] = {0, 0, 0, 0, 0};
#pragma unroll 1
    for (size_t k = 0; k < steps; k++) {
        const size_t j = s + k * parts;
        const bool have = j < terms;
        u64 xa[5], xb[5];
        load(k, j, have, xa, xb);
        if (have) {
            u64 q[5];
            sc_muladd_limbs52(q, xa, xb, r);
#pragma unroll
            for (int i = 0; i < 5; i++) r[i] = q[i];
        }
    }
    return fe_from_limbs52(r);
#endif
    scv_cols c;
    scv_cols_zero(c);
    u32 pending = 0;                                                                      // products since the last carry pass
#pragma unroll 1
    for (size_t k = 0; k < steps; k++) {
        const size_t j = s + k * parts;
        const bool have = j < terms;
        u64 xa[5], xb[5];
        load(k, j, have, xa, xb);
        if (have) {
            if (pending == SCV_CARRY_EVERY) {
                scv_cols_carry(c);
                pending = 0;
            }
            scv_cols_mac(c, fe_from_limbs52(xa), fe_from_limbs52(xb));
            pending++;
        }
    }
    return scv_cols_fold(c, steps <= SCV_NOHI_MAX);
}
template <class LOAD>
ZC_DI fe scv_slice_sum(size_t terms, size_t parts, size_t s, size_t steps, LOAD&& load)
{
    scv_cols c;
    scv_cols_zero(c);
#pragma unroll 1
    for (size_t k = 0; k < steps; k++) {
        const size_t j = s + k * parts;
        const bool have = j < terms;
        u64 xa[5];
        load(k, j, have, xa);
        if (have) {
            const fe a = fe_from_limbs52(xa);
#pragma unroll
            for (int i = 0; i < 9; i++) c.t[i] += a.v[i];                                 // below 2^31 limbs of 29 bits
        }
    }
    return scv_cols_fold(c, true);                                                        // X < 2^31 2^260
}
// The same for the short slices of the block form (steps <= SCV_NOHI_MAX, fewer products than a carry pass waits for): the steps
// unrolled, so that a loader may keep a lane's records in registers.
static_assert(SCV_NOHI_MAX <= SCV_CARRY_EVERY, "a block slice needs no carry pass");
template <bool DOT, class LOAD>
ZC_DI fe scv_block_slice(size_t terms, size_t parts, size_t s, size_t steps, LOAD&& load)
{
#if ZC_SCV_DOT_CHAINED
    if (DOT) {
        u64 r[5] = {0, 0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < (int)SCV_NOHI_MAX; k++) {
            const size_t j = s + (size_t)k * parts;
            const bool have = (size_t)k < steps && j < terms;
            u64 xa[5], xb[5], q[5];
            load(k, j, have, xa, xb);
            if (!have) continue;
            sc_muladd_limbs52(q, xa, xb, r);
#pragma unroll
            for (int i = 0; i < 5; i++) r[i] = q[i];
        }
        return fe_from_limbs52(r);
    }
#endif
    scv_cols c;
    scv_cols_zero(c);
    ZC_ASSERT(steps <= SCV_NOHI_MAX);
#pragma unroll
    for (int k = 0; k < (int)SCV_NOHI_MAX; k++) {
        const size_t j = s + (size_t)k * parts;
        const bool have = (size_t)k < steps && j < terms;
        u64 xa[5], xb[5];
        load(k, j, have, xa, xb);
        if (have) {
            const fe a = fe_from_limbs52(xa);
            if (DOT) {
                scv_cols_mac(c, a, fe_from_limbs52(xb));
            } else {
#pragma unroll
                for (int i = 0; i < 9; i++) c.t[i] += a.v[i];
            }
        }
    }
    return scv_cols_fold(c, true);
}
// One tree level over w partials: element s < w / 2 becomes q[s] + q[s + half] with half = scv_tree_half(w); the middle element of
// an odd level, q[half - 1], stays as it is; the next level has `half` elements.
ZC_DI size_t scv_tree_half(size_t w) { return (w + 1) / 2; }

// The powers of one lane: lane l of a group of G (a power of two) holds x^l, from the bits of l, and x^G, the last square of the
// same ladder; emit(k, j, have, limbs) takes x^j, j = l + k G, in every one of the `steps` steps (have false past the row's end).
template <class EMIT>
ZC_DI void scv_pow_lane(const u64 (&x)[5], u32 l, u32 G, u32 terms, u32 steps, EMIT&& emit)
{
    typedef ModL F;
    const fe xm = mont_to<F>(fe_from_limbs52(x));                                        // any 260-bit pattern: below 3 L
    fe acc = fe_one_m<F>();                                                               // x^0 = 1, also for x = 0 mod L
    fe sq = xm;
#pragma unroll 1
    for (u32 g = 1; g < G; g <<= 1) {
        if (l & g) acc = mont_mul<F>(acc, sq);
        sq = mont_sqr<F>(sq);
    }
#pragma unroll 1
    for (u32 k = 0; k < steps; k++) {
        const u32 j = l + k * G;
        u64 r[5];
        fe_to_limbs52(r, fe_canon_from_mont<F>(acc));
        emit(k, j, j < terms, r);
        if (k + 1 < steps) acc = mont_mul<F>(acc, sq);
    }
}

}  // namespace zc

// the kernels: hipcc only (the host emulation of the test tier builds the device functions above with a C++ compiler)
#if defined(__HIPCC__)
#include "zc_kernels.hip.h"

namespace zc {

#define ZC_KERNEL_SCV extern "C" __global__ __launch_bounds__(SCV_BLOCK)
constexpr int SCV_REC_WORDS = SCV_BLOCK * 5;                  // 64-bit words of a step's 256 records

ZC_DI void scv_partial_put(u32* __restrict__ q, size_t e, const fe& a)
{
#pragma unroll
    for (int i = 0; i < 9; i++) q[(size_t)i * SCV_BLOCK + e] = a.v[i];
}
ZC_DI fe scv_partial_get(const u32* __restrict__ q, size_t e)
{
    fe a;
#pragma unroll
    for (int i = 0; i < 9; i++) a.v[i] = q[(size_t)i * SCV_BLOCK + e];
    return a;
}
// The tree over partials in LDS, `width` per row, rows side by side: the calling lane is element s of the row whose first lane is
// `base` (s >= width: a lane without a partial).  Leaves the row's sum in the lane with s == 0.  Every lane of the workgroup calls it.
ZC_DI void scv_tree_in_block(u32* __restrict__ q, fe& acc, size_t base, size_t s, size_t width)
{
    if (width <= 1) return;
    __syncthreads();                                       // the buffer's last readers are through
    scv_partial_put(q, threadIdx.x, acc);
#pragma unroll 1
    for (size_t w = width; w > 1;) {
        const size_t half = scv_tree_half(w);
        __syncthreads();
        const bool mine = s < w / 2;
        if (mine) acc = scv_pair(acc, scv_partial_get(q, base + s + half));
        __syncthreads();
        if (mine) scv_partial_put(q, threadIdx.x, acc);
        w = half;
    }
}
ZC_DI void scv_row_store(u64* __restrict__ out, const fe& a)
{
    u64 r[5];
    fe_to_limbs52(r, a);
#pragma unroll
    for (int i = 0; i < 5; i++) out[i] = r[i];
}
// The block form (terms <= SCV_BLOCK_TERMS_MAX; parts = 1, 4, 16, 64 or 256 with terms <= 4 parts): workgroup g holds the
// 256 / parts rows g * (256 / parts) ..., lane t slice t % parts of row t / parts.  The rows of a workgroup are one contiguous
// block of at most SCV_STAGE records: it comes in whole, with 8-byte loads along the addresses, and a lane picks its at most four
// records out of LDS.  The dot product brings in the block of a, keeps the lane's records in registers, then the block of b (a
// shared b: its one row) through the same 40 KB.
template <bool DOT>
ZC_DI void scv_rows_block(const u64* __restrict__ a, const u64* __restrict__ b, bool shared_b, u32 terms, u32 parts, u64* __restrict__ out, size_t n)
{
    __shared__ u64 st[SCV_STAGE * 5];
    const u32 t = threadIdx.x;
    const int psh = __builtin_ctz(parts);
    const u32 rpb = (u32)SCV_BLOCK >> psh, r = t >> psh, s = t & (parts - 1);
    const size_t row0 = (size_t)blockIdx.x * rpb, row = row0 + r;
    const u32 rows = n - row0 < rpb ? (u32)(n - row0) : rpb;                         // the grid has no workgroup without a row
    const bool valid = r < rows;
    const u32 steps = scv_fold_steps(terms, parts), words = rows * terms * 5;        // <= SCV_STAGE * 5
    const u64* src = a + row0 * terms * 5;
    for (u32 v = t; v < words; v += SCV_BLOCK) st[v] = src[v];
    __syncthreads();
    u64 ra[SCV_NOHI_MAX][5];
    if (DOT) {
#pragma unroll
        for (int k = 0; k < (int)SCV_NOHI_MAX; k++) {
            const u32 j = s + (u32)k * parts;
#pragma unroll
            for (int i = 0; i < 5; i++) ra[k][i] = valid && (u32)k < steps && j < terms ? st[5 * (r * terms + j) + i] : 0;
        }
        __syncthreads();
        const u32 bwords = shared_b ? terms * 5 : words;
        src = b + (shared_b ? 0 : row0 * terms * 5);
        for (u32 v = t; v < bwords; v += SCV_BLOCK) st[v] = src[v];
        __syncthreads();
    }
    fe acc = scv_block_slice<DOT>(valid ? terms : 0, parts, s, steps, [&](int k, size_t j, bool have, u64 (&xa)[5], u64 (&xb)[5]) {
        const u32 at = 5 * ((u32)scv_b_record(DOT && shared_b, r, terms, j));
#pragma unroll
        for (int i = 0; i < 5; i++) {
            xa[i] = DOT ? ra[k][i] : have ? st[at + i] : 0;
            xb[i] = DOT && have ? st[at + i] : 0;
        }
    });
    static_assert(sizeof(st) >= 9 * SCV_BLOCK * sizeof(u32), "the records' buffer holds the tree's partials");
    scv_tree_in_block(reinterpret_cast<u32*>(st), acc, t - s, s, parts);
    if (valid && s == 0) scv_row_store(out + 5 * row, acc);
}
ZC_KERNEL_SCV void k_sc_rowsum(const u64* a, u32 terms, u32 parts, u64* out, size_t n) { scv_rows_block<false>(a, nullptr, false, terms, parts, out, n); }
ZC_KERNEL_SCV void k_sc_rowdot(const u64* a, const u64* b, u32 shared_b, u32 terms, u32 parts, u64* out, size_t n)
{
    scv_rows_block<true>(a, b, shared_b != 0, terms, parts, out, n);
}
// The long forms: 256 slices of one row per workgroup, two steps of 256 consecutive records staged at a time.  ROW (TWO false,
// parts = SCV_BLOCK): workgroup g is row g and writes its result.  TWO: workgroup g holds slices (g % bpr) * SCV_BLOCK ... of row
// g / bpr, bpr = parts / SCV_BLOCK (any count), and leaves one partial in the workspace.  Both grids are exact.
template <bool DOT, bool TWO>
ZC_DI void scv_rows_long(const u64* __restrict__ a, const u64* __restrict__ b, bool shared_b, u32 terms, u32 parts, u64* __restrict__ out, u32* __restrict__ ws)
{
    constexpr u32 STEP_WORDS = 5 * SCV_BLOCK, STAGE_WORDS = STEP_WORDS * (u32)SCV_LONG_STAGE_STEPS;
    __shared__ u64 sa[STAGE_WORDS];
    __shared__ u64 sb[DOT ? STAGE_WORDS : 1];
    const u32 t = threadIdx.x;
    const u32 steps = scv_fold_steps(terms, parts);
    const u32 bpr = TWO ? parts / (u32)SCV_BLOCK : 1;
    const size_t row = TWO ? blockIdx.x / bpr : blockIdx.x;
    const u32 slice0 = TWO ? (blockIdx.x % bpr) * (u32)SCV_BLOCK : 0;
    const u32 s = slice0 + t;
    // steps k, k + 1 of the workgroup: word w of lane l's record of step k + kk, consecutive lanes of the copy along the records
    const auto stage = [&](u32 k) {
        __syncthreads();                                     // the last steps' records have been read
#pragma unroll
        for (u32 i = 0; i < STAGE_WORDS / SCV_BLOCK; i++) {
            const u32 v = t + i * SCV_BLOCK, kk = v / STEP_WORDS, lw = v % STEP_WORDS, l = lw / 5, w = lw % 5;
            const u32 lj = slice0 + l + (k + kk) * parts;    // (k + kk) * parts < terms + 2 parts < 2^32
            if (k + kk < steps && lj < terms) {
                sa[v] = a[5 * (row * terms + lj) + w];
                if (DOT) sb[v] = b[5 * scv_b_record(shared_b, row, terms, lj) + w];
            }
        }
        __syncthreads();
    };
    const auto at = [&](size_t k) { return ((u32)k % (u32)SCV_LONG_STAGE_STEPS) * STEP_WORDS + 5 * t; };
    fe acc;
    if (DOT) {
        acc = scv_slice_dot(terms, parts, s, steps, [&](size_t k, size_t, bool have, u64 (&xa)[5], u64 (&xb)[5]) {
            if (k % SCV_LONG_STAGE_STEPS == 0) stage((u32)k);
#pragma unroll
            for (int i = 0; i < 5; i++) {
                xa[i] = have ? sa[at(k) + i] : 0;
                xb[i] = have ? sb[at(k) + i] : 0;
            }
        });
    } else {
        acc = scv_slice_sum(terms, parts, s, steps, [&](size_t k, size_t, bool have, u64 (&xa)[5]) {
            if (k % SCV_LONG_STAGE_STEPS == 0) stage((u32)k);
#pragma unroll
            for (int i = 0; i < 5; i++) xa[i] = have ? sa[at(k) + i] : 0;
        });
    }
    static_assert(sizeof(sa) >= 9 * SCV_BLOCK * sizeof(u32), "the records' buffer holds the tree's partials");
    scv_tree_in_block(reinterpret_cast<u32*>(sa), acc, 0, t, SCV_BLOCK);
    if (t != 0) return;
    if (TWO) {
        u32* o = ws + (size_t)blockIdx.x * SCV_PARTIAL_WORDS;
#pragma unroll
        for (int i = 0; i < 9; i++) o[i] = acc.v[i];
    } else {
        scv_row_store(out + 5 * row, acc);
    }
}
ZC_KERNEL_SCV void k_sc_rowsum_long(const u64* a, u32 terms, u32 parts, u64* out) { scv_rows_long<false, false>(a, nullptr, false, terms, parts, out, nullptr); }
ZC_KERNEL_SCV void k_sc_rowsum_part(const u64* a, u32 terms, u32 parts, u32* ws) { scv_rows_long<false, true>(a, nullptr, false, terms, parts, nullptr, ws); }
ZC_KERNEL_SCV void k_sc_rowdot_long(const u64* a, const u64* b, u32 shared_b, u32 terms, u32 parts, u64* out)
{
    scv_rows_long<true, false>(a, b, shared_b != 0, terms, parts, out, nullptr);
}
ZC_KERNEL_SCV void k_sc_rowdot_part(const u64* a, const u64* b, u32 shared_b, u32 terms, u32 parts, u32* ws)
{
    scv_rows_long<true, true>(a, b, shared_b != 0, terms, parts, nullptr, ws);
}
// Partial e of the bpr partials of a row in the workspace.
ZC_DI fe scv_ws_get(const u32* __restrict__ ws, size_t e)
{
    fe a;
#pragma unroll
    for (int i = 0; i < 9; i++) a.v[i] = ws[e * SCV_PARTIAL_WORDS + i];
    return a;
}
// The second kernel of the TWO form: workgroup i adds the bpr (2 .. SCV_MAX_BPR) partials of row i: lane t the partials
// t, t + 256, ..., then the tree over the first min(bpr, 256) lanes.
ZC_KERNEL_SCV void k_sc_rows_finish(const u32* ws, u32 bpr, u64* out, size_t n)
{
    __shared__ u32 q[9 * SCV_BLOCK];
    const size_t t = threadIdx.x, row = blockIdx.x;
    if (row >= n) return;                                    // the whole workgroup
    fe acc = fe_zero();
#pragma unroll 1
    for (size_t e = t; e < bpr; e += SCV_BLOCK) acc = scv_pair(acc, scv_ws_get(ws, row * bpr + e));
    scv_tree_in_block(q, acc, 0, t, bpr < (u32)SCV_BLOCK ? bpr : (u32)SCV_BLOCK);
    if (t == 0) scv_row_store(out + 5 * row, acc);
}

// Powers.  G < SCV_BLOCK: workgroup g holds rows g * (SCV_BLOCK / G) ..., lane t is lane t % G of row t / G, steps <= 4, and the
// workgroup's rows are one contiguous block of the output, staged whole.  G >= SCV_BLOCK: workgroup g is lanes
// (g % (G / SCV_BLOCK)) * SCV_BLOCK ... of row g / (G / SCV_BLOCK); a step is 256 consecutive records, four steps go out together.
ZC_KERNEL_SCV void k_sc_powers(const u64* __restrict__ x, u32 terms, u32 G, u64* __restrict__ out, size_t n)
{
    __shared__ u64 st[SCV_POW_STAGE * 5];
    const u32 t = threadIdx.x;
    const bool small = G < (u32)SCV_BLOCK;
    const int gsh = __builtin_ctz(G);
    const u32 bpr = small ? 1 : G >> 8;
    const size_t row0 = small ? (size_t)blockIdx.x << (8 - gsh) : blockIdx.x / bpr;
    const u32 lane0 = small ? 0 : (blockIdx.x % bpr) << 8;
    const size_t row = small ? row0 + (t >> gsh) : row0;
    const u32 l = small ? t & (G - 1) : lane0 + t;
    const bool valid = row < n;
    const u32 steps = scv_fold_steps(terms, G);
    u64 xl[5];
#pragma unroll
    for (int i = 0; i < 5; i++) xl[i] = valid ? x[5 * row + i] : 0;
    scv_pow_lane(xl, l, G, valid ? terms : 0, steps, [&](u32 k, u32 j, bool have, const u64 (&r)[5]) {
        const u32 slot = small ? (t >> gsh) * terms + j : (k % (u32)SCV_POW_STAGE_STEPS) * (u32)SCV_BLOCK + t;
        if (have) {
#pragma unroll
            for (int i = 0; i < 5; i++) st[5 * (size_t)slot + i] = r[i];
        }
        if ((k + 1) % (u32)SCV_POW_STAGE_STEPS != 0 && k + 1 != steps) return;          // uniform: every lane walks the same steps
        __syncthreads();
        if (small) {
            const size_t rows = n - row0 < ((size_t)SCV_BLOCK >> gsh) ? n - row0 : (size_t)SCV_BLOCK >> gsh;
            const size_t words = rows * terms * 5;                                       // <= SCV_POW_STAGE * 5
            u64* o = out + row0 * terms * 5;
            for (size_t v = t; v < words; v += SCV_BLOCK) o[v] = st[v];
        } else {
            const u32 k0 = k - k % (u32)SCV_POW_STAGE_STEPS;
            u64* o = out + row0 * terms * 5;
            for (u32 v = t; v < (u32)SCV_POW_STAGE * 5; v += SCV_BLOCK) {
                const u32 kk = k0 + v / (5 * (u32)SCV_BLOCK), w = v % (5 * (u32)SCV_BLOCK);   // step, word inside the step's 256 records
                const size_t jw = ((size_t)lane0 + (size_t)kk * G) * 5 + w;
                if (kk <= k && jw < (size_t)terms * 5) o[jw] = st[v];
            }
        }
        __syncthreads();
    });
}

}  // namespace zc
#endif
