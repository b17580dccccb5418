// zc_sum.hip.h -- point sums: out[i] = P_i0 + P_i1 + ... over rows of any length (zerocaf_hip_ext_sum_rows.h), and the same
// between the Ristretto codecs.
//
// The order of association is the plan's (zc_sum_plan.h) and a function of `terms` alone: P = sum_parts(terms) slices, slice s
// the points s, s + P, s + 2 P, ... folded from the left, then the P partial sums combined by adjacent pairs, level by level.
// Every addition is ptm_add (zc_curve.hip.h): the field values of the reference's unified addition (edwards.rs:465-489), so the
// canonical limbs of a row are those of the oracle's ed_add applied in that order, whatever the launch form.
//   per point      one addition of 9 multiplications (+ 4 to bring the record into the Montgomery domain)
//   wire form      + ris_decompress per point, ris_compress per row
// Lane mapping: lane l of a workgroup is (row l / W, slice l % W) of its W = min(P, 256) slices, so at every fold step
// neighbouring lanes want neighbouring 160-byte records (P = 1: records `terms` apart).  The workgroup's 256 records of a step come
// in through LDS with 8-byte loads that run along each record, not as 64 scattered 40-byte reads per instruction; the same 40 KB
// then holds the partials of the tree.
#pragma once
#include "zc_curve.hip.h"
#include "zc_sum_plan.h"

namespace zc {

// Keeps a per-lane value in a vector register from here on.  A lane mask (a bool) or a uniform pointer carried across the wire
// fold's loop costs two scalar registers each, and that loop has none to spare: the decode's constants fill the scalar file.
#if defined(__HIP_DEVICE_COMPILE__)
#define ZC_SUM_IN_VGPR(x) asm volatile("" : "+v"(x))
#define ZC_SUM_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)      // a value kept per lane that is the same in every active lane
#else
#define ZC_SUM_IN_VGPR(x) ((void)(x))
#define ZC_SUM_UNIFORM(x) (x)
#endif

// A partial sum as it lies in LDS or in the workspace: the 4 x 9 words of (Y-X, Y+X, Z, T), then the accept bit.  Word w of
// element e is q[e * es + w * ws] (LDS: es = 1, ws = SUM_BLOCK, no bank conflicts; workspace: es = SUM_PARTIAL_WORDS, ws = 1).
ZC_DI void sum_partial_put(u32* __restrict__ q, size_t e, size_t es, size_t ws, const ptm& a, bool ok)
{
    u32* o = q + e * es;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        o[(size_t)i * ws] = a.Ym.v[i];
        o[(size_t)(9 + i) * ws] = a.Yp.v[i];
        o[(size_t)(18 + i) * ws] = a.Z.v[i];
        o[(size_t)(27 + i) * ws] = a.T.v[i];
    }
    o[36 * ws] = ok ? 1u : 0u;
}
ZC_DI ptm sum_partial_get(const u32* __restrict__ q, size_t e, size_t es, size_t ws, bool& ok)
{
    const u32* o = q + e * es;
    ptm a;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        a.Ym.v[i] = o[(size_t)i * ws];
        a.Yp.v[i] = o[(size_t)(9 + i) * ws];
        a.Z.v[i] = o[(size_t)(18 + i) * ws];
        a.T.v[i] = o[(size_t)(27 + i) * ws];
    }
    ok = o[36 * ws] != 0;
    return a;
}

// Slice s of a row of `terms` points cut into `parts`: the points s, s + parts, ... folded from the left, starting FROM THE FIRST
// POINT (a row of one term is its point, not identity + point: another representative).  load(k, j, have) -> pt brings point j of
// the row in step k; it is called in every one of the `steps` steps, also past the slice's end (have false: the staged loader of the
// kernels has barriers inside, and every lane of a workgroup walks the same steps).  A lane without a row passes terms = 0.
template <class LOAD>
ZC_DI ptm sum_slice_fold(size_t terms, size_t parts, size_t s, size_t steps, LOAD&& load)
{
    ptm acc = ptm_from_pt(pt_identity());
#pragma unroll 1
    for (size_t k = 0; k < steps; k++) {
        const size_t j = s + k * parts;
        const bool have = j < terms;
        const pt P = load(k, j, have);
        if (have) acc = k == 0 ? ptm_from_pt(P) : ptm_add(acc, ptm_from_pt(P));
    }
    return acc;
}
// fp_sqrt_ratio_i(out, 1, v) (zc_curve.hip.h) without its products by the constant 1: the same root and the same verdict.  In
// the fold loop below the general form's products of two constants (u i, the canonical u) are loop-invariant, get hoisted and
// stay live in 160 scalar registers across the whole decode, which then spills; here there is none.
ZC_DI bool sum_inv_sqrt_i(fe& out, const fe& v)
{
    const fe i_m = fe_const<FP>(ModP::SQRT_M1_M), one = fe_one_m<FP>();
    const fe v3 = fp_mul(fp_sqr(v), v);
    const fe v7 = fp_mul(fp_sqr(v3), v);
    fe r = fp_mul(v3, fp_pow_p58(v7));
    const fe check = fp_mul(v, fp_sqr(r));
    const bool correct = fp_is_zero(fp_sub(check, one));
    const bool flipped = fe_is_zero_canon(fp_canon(fe_add(check, one)));          // check == -1
    const bool flipped_i = fe_is_zero_canon(fp_canon(fe_add(check, i_m)));        // check == -i
    r = fe_select(flipped || flipped_i, fp_mul(r, i_m), r);
    out = fp_abs(r);
    return correct || flipped;
}
// ris_decompress (zc_curve.hip.h; ristretto.rs:96-154) on that root: the same point, limb for limb, and the same verdict.
ZC_DI bool sum_ris_decode(pt& out, const u64 (&w)[4])
{
    const fe raw = fe_from_words256(w);
    const bool s_ok = words256_is_positive(raw);
    const fe one = fe_one_m<FP>();
    const fe s = mont_to<FP>(raw);
    const fe ss = fp_sqr(s);
    const fe u1 = fp_sub(one, ss);
    const fe u2 = fe_add(one, ss);
    const fe u2sq = fp_sqr(u2);
    const fe v = fp_sub(fp_neg(fp_mul(fe_const<FP>(ModP::D_M), fp_sqr(u1))), u2sq);
    fe I;
    const bool was_sq = sum_inv_sqrt_i(I, fp_mul(v, u2sq));
    const fe Dx = fp_mul(I, u2);
    const fe Dy = fp_mul(fp_mul(I, Dx), v);
    out.X = fp_abs(fp_mul(fe_add(s, s), Dx));
    out.Y = fp_mul(u1, Dy);
    out.Z = one;
    out.T = fp_mul(out.X, out.Y);
    return s_ok && was_sq && fp_is_positive(out.T) && !fp_is_zero(out.Y);
}
// The same over encodings: load(w, j) brings the 32 bytes of point j; ok leaves as the AND of the slice's accept bits.
// An encoding that does not decode adds what the decoder left (deterministic, and the row's bytes are zeroed at the end).
template <class LOAD>
ZC_DI ptm sum_wire_slice_fold(u32 terms, u32 parts, u32 s, u32 steps, bool& ok, LOAD&& load)   // (n * terms < 2^31: 32-bit indices)
{
    ptm acc = ptm_from_pt(pt_identity());
    u32 okw = 1, fresh = 1, j = s;                           // the accept bit and "no point yet" as words of the lane, not as lane masks
#pragma unroll 1
    for (u32 left = steps; ZC_SUM_UNIFORM(left) != 0; left--, j += parts) {
        ZC_SUM_IN_VGPR(okw);
        ZC_SUM_IN_VGPR(fresh);
        ZC_SUM_IN_VGPR(left);
        if (j < terms) {
            u64 w[4];
            load(w, j);
            pt P;
            const bool dec = sum_ris_decode(P, w);
            okw = okw & (dec ? 1u : 0u);
            const ptm m = ptm_from_pt(P);
            acc = ZC_SUM_UNIFORM(fresh) ? m : ptm_add(acc, m);      // every lane that has a point has its first in step 0
            fresh = 0;
        }
    }
    ok = okw != 0;
    return acc;
}
// One tree level over an array of partials: element s of the next level is q[2 s] + q[2 s + 1], accepted when both are.
ZC_DI ptm sum_tree_pair(const u32* __restrict__ q, size_t s, size_t es, size_t ws, bool& ok)
{
    bool oa, ob;
    const ptm a = sum_partial_get(q, 2 * s, es, ws, oa);
    const ptm b = sum_partial_get(q, 2 * s + 1, es, ws, ob);
    ok = oa && ob;
    return ptm_add(a, b);
}
// Fold steps every lane of a launch walks through: the longest slice's (slice 0), ceil(terms / parts).
ZC_DI u32 sum_fold_steps(u32 terms, u32 parts) { return (terms + parts - 1) / parts; }
// The tree runs while a level is wider than this.
ZC_DI bool sum_tree_more(size_t width) { return width > 1; }

// How a row leaves: the point with canonical limbs, or its encoding (32 zero bytes when a term was refused).
ZC_DI void sum_row_store(u64* __restrict__ out, const ptm& a) { pt_store(out, ptm_to_pt(a)); }
ZC_DI void sum_row_encode(u64 (&w)[4], const ptm& a, bool ok)
{
    fe_to_words256(w, ris_compress(ptm_to_pt(a)));
    if (!ok) w[0] = w[1] = w[2] = w[3] = 0;
}

}  // namespace zc

// the kernels: hipcc only (the host emulation of the test tier builds the device functions above with a C++ compiler)
#if defined(__HIPCC__)
#include "zc_kernels.hip.h"

namespace zc {

#define ZC_KERNEL_SUM extern "C" __global__ __launch_bounds__(SUM_BLOCK)
#ifndef ZC_KERNEL_SUM_WIRE
#define ZC_KERNEL_SUM_WIRE ZC_KERNEL_SUM
#endif
constexpr int SUM_LDS_WORDS = SUM_BLOCK * 40;                 // 40 KB: 256 records of 160 bytes, or 256 partials of 37 words

// The tree over the workgroup's partials, `width` (a power of two, <= SUM_BLOCK) per row, rows side by side: lane t is element
// t % width of row t / width.  Leaves the row's sum in the lane with t % width == 0.  Every lane of the workgroup calls it.
ZC_DI void sum_tree_in_block(u32* __restrict__ q, ptm& acc, bool& ok, size_t width)
{
    const size_t t = threadIdx.x, s = t & (width - 1), base = t - s;
    if (!sum_tree_more(width)) return;
    __syncthreads();                                       // the buffer's last readers are through
    sum_partial_put(q, t, 1, SUM_BLOCK, acc, ok);
#pragma unroll 1
    for (size_t w = width; sum_tree_more(w); w >>= 1) {
        __syncthreads();
        const bool mine = s < (w >> 1);
        if (mine) acc = sum_tree_pair(q + base, s, 1, SUM_BLOCK, ok);
        __syncthreads();
        if (mine) sum_partial_put(q, t, 1, SUM_BLOCK, acc, ok);
    }
}
// The first kernel, one instance per form so that each keeps only its own arguments live.  GROUP (TWO false, parts <= SUM_BLOCK):
// workgroup b holds rows b * (SUM_BLOCK / parts) ..., lane t slice t % parts of row t / parts, and writes the rows' results.
// TWO (parts > SUM_BLOCK): workgroup b holds slices (b % bpr) * SUM_BLOCK ... of row b / bpr, bpr = parts / SUM_BLOCK, and leaves
// one partial in the workspace; its grid is exactly n * bpr.  Width, steps and bpr follow from terms and parts here.
template <bool WIRE, bool TWO>
ZC_DI void sum_rows_first(const void* in, u32 terms, u32 parts, void* out, uint8_t* okv, u32* ws, size_t n)
{
    __shared__ __attribute__((aligned(16))) u32 lds[SUM_LDS_WORDS];
    const u32 t = threadIdx.x;                                                      // (terms, parts and slices fit 32 bits: n * terms < 2^31)
    const u32 width = TWO ? (u32)SUM_BLOCK : parts;                                  // slices of a row in this workgroup
    const u32 steps = sum_fold_steps(terms, parts);
    const int wsh = __builtin_ctz(width), bsh = __builtin_ctz(parts) - 8;            // powers of two; SUM_BLOCK = 2^8
    const size_t row0 = TWO ? blockIdx.x >> bsh : (size_t)blockIdx.x << (8 - wsh);   // the workgroup's first row
    const u32 slice0 = TWO ? (blockIdx.x & ((1u << bsh) - 1)) << 8 : 0;              // ... and first slice
    const size_t row = row0 + (t >> wsh);
    const u32 s = slice0 + (t & (width - 1));
    const bool valid = TWO || row < n;
    ptm acc;
    bool ok = true;
    // where this lane's result goes, if it has one (0: none): formed before the fold and kept per lane, so that neither the
    // output pointers nor the validity mask stay in scalar registers across it
    uintptr_t dst = 0, okd = 0;
    u32 pvw = parts;
    if (valid && (t & (width - 1)) == 0) {
        dst = TWO ? reinterpret_cast<uintptr_t>(ws + (size_t)blockIdx.x * SUM_PARTIAL_WORDS)
                  : reinterpret_cast<uintptr_t>(out) + (WIRE ? 32 : 160) * row;
        okd = okv ? reinterpret_cast<uintptr_t>(okv + row) : 0;
    }
    if (WIRE) {
        ZC_SUM_IN_VGPR(dst);
        ZC_SUM_IN_VGPR(okd);
        u32 mine = valid ? terms : 0;
        ZC_SUM_IN_VGPR(mine);
        ZC_SUM_IN_VGPR(pvw);                                 // parts rides through the fold per lane too
        const uint8_t* enc = static_cast<const uint8_t*>(in) + (size_t)32 * terms * (valid ? row : 0);
        acc = sum_wire_slice_fold(mine, pvw, s, steps, ok, [&](u64 (&w)[4], size_t j) { load_words256(w, enc + (size_t)32 * j); });
    } else {
        const u64* pts = static_cast<const u64*>(in);
        u64* stage = reinterpret_cast<u64*>(lds);
        acc = sum_slice_fold(valid ? terms : 0, parts, s, steps, [&](size_t k, size_t, bool have) {
            __syncthreads();                                 // the last step's records have been read
#pragma unroll 4
            for (int i = 0; i < 20; i++) {
                const u32 v = (u32)t + (u32)i * SUM_BLOCK, l = v / 20, w = v % 20;       // word w of lane l's record
                const size_t lrow = row0 + (l >> wsh);
                const u32 lj = slice0 + (l & (width - 1)) + (u32)k * parts;
                if ((TWO || lrow < n) && lj < terms) stage[v] = pts[20 * (lrow * terms + lj) + w];
            }
            __syncthreads();
            return have ? pt_load(stage + 20 * t) : pt_identity();
        });
    }
    sum_tree_in_block(lds, acc, ok, TWO ? (u32)SUM_BLOCK : WIRE ? (u32)ZC_SUM_UNIFORM(pvw) : width);
    if (!dst) return;
    if (TWO) {
        sum_partial_put(reinterpret_cast<u32*>(dst), 0, SUM_PARTIAL_WORDS, 1, acc, ok);
    } else if (WIRE) {
        u64 w[4];
        sum_row_encode(w, acc, ok);
        store_words256(reinterpret_cast<uint8_t*>(dst), w);
        if (okd) *reinterpret_cast<uint8_t*>(okd) = ok ? 1 : 0;
    } else {
        sum_row_store(reinterpret_cast<u64*>(dst), acc);
    }
}
ZC_KERNEL_SUM void k_ed_rowsum(const u64* points, u32 terms, u32 parts, u64* out, size_t n) { sum_rows_first<false, false>(points, terms, parts, out, nullptr, nullptr, n); }
ZC_KERNEL_SUM void k_ed_rowsum_part(const u64* points, u32 terms, u32 parts, u32* ws) { sum_rows_first<false, true>(points, terms, parts, nullptr, nullptr, ws, 0); }
ZC_KERNEL_SUM_WIRE void k_ris_rowsum(const uint8_t* in, u32 terms, u32 parts, uint8_t* out, uint8_t* ok, size_t n) { sum_rows_first<true, false>(in, terms, parts, out, ok, nullptr, n); }
ZC_KERNEL_SUM_WIRE void k_ris_rowsum_part(const uint8_t* in, u32 terms, u32 parts, u32* ws) { sum_rows_first<true, true>(in, terms, parts, nullptr, nullptr, ws, 0); }
// The second kernel of the TWO form: workgroup i finishes the bpr (a power of two, 2 .. SUM_BLOCK) partials of row i.
template <bool WIRE>
ZC_DI void sum_rows_finish(const u32* ws, u32 bpr, void* out, uint8_t* okv, size_t n)
{
    __shared__ u32 lds[SUM_BLOCK * 37];
    const size_t t = threadIdx.x, row = blockIdx.x;
    if (row >= n) return;                                    // the whole workgroup
    ptm acc = ptm_from_pt(pt_identity());
    bool ok = true;
    if (t < bpr) acc = sum_partial_get(ws, row * bpr + t, SUM_PARTIAL_WORDS, 1, ok);
    sum_tree_in_block(lds, acc, ok, bpr);
    if (t != 0) return;
    if (WIRE) {
        u64 w[4];
        sum_row_encode(w, acc, ok);
        store_words256(static_cast<uint8_t*>(out) + 32 * row, w);
        if (okv) okv[row] = ok ? 1 : 0;
    } else {
        sum_row_store(static_cast<u64*>(out) + 20 * row, acc);
    }
}
ZC_KERNEL_SUM void k_ed_rowsum_finish(const u32* ws, u32 bpr, u64* out, size_t n) { sum_rows_finish<false>(ws, bpr, out, nullptr, n); }
ZC_KERNEL_SUM void k_ris_rowsum_finish(const u32* ws, u32 bpr, uint8_t* out, uint8_t* ok, size_t n) { sum_rows_finish<true>(ws, bpr, out, ok, n); }

}  // namespace zc
#endif
