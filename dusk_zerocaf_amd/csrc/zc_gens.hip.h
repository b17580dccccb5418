// zc_gens.hip.h -- generator sets: out[i] = sum_j k_ij * G_j over 1..8 caller-supplied fixed points (zerocaf_hip_ext_gens.h).
//
// The comb of the curve basepoint (zc_curve.hip.h: comb_table_column, scalar_recode256, base_mul_onto) over any point: per
// generator a table T_j[w][e] = (e+1) * 256^w * G_j of 33 x 128 cached affine records (540 672 bytes), the tables of a set one
// behind the other.  A row walks its terms one after another: recode scalar j into the lane's nine LDS words, then up to 33
// mixed additions from table j on top of the running sum.  No doublings, no per-row table, no ring slot.
//   per term   33 mixed additions of 7 multiplications                      231 multiplications
//   wire form  + ris_compress (one square-root power)
// against 1827 + 567 t for zc_ed_lincomb with the generators tiled into every row.
//
// Like base_mul: the same group element as the reference's ((k_0 G_0 + k_1 G_1) + ...), another projective representative,
// deterministic limbs that depend on the row and the set only.  Nothing here is constant-time: the trip count is the row's
// top digit and the records read are the digits'.
#pragma once
#include "zc_curve.hip.h"

namespace zc {

constexpr int GENS_MAX = 8;                                                               // ZC_GENS_MAX of the header
constexpr size_t GENS_TABLE_WORDS = (size_t)ZC_BASE_WINDOWS * ZC_BASE_ENTRIES * 32;      // one generator's comb

// The generator at p (20 limbs; T is not read) as (X/Z, Y/Z, 1, XY/Z^2).  false: not a point of the curve by value -- the
// curve equation fails or Z is 0 mod p (Z = 0 satisfies the projective equation whenever X Y = 0) -- and G holds no point.
ZC_DI bool gens_normalise(pt& G, const u64* __restrict__ p)
{
    pt P;
    P.X = fe_load_mont<FP>(p);
    P.Y = fe_load_mont<FP>(p + 5);
    P.Z = fe_load_mont<FP>(p + 10);
    const bool ok = ed_is_valid(P) && !fp_is_zero(P.Z);
    const fe zi = fp_invert(P.Z);
    G.X = fp_mul(P.X, zi);
    G.Y = fp_mul(P.Y, zi);
    G.Z = fe_one_m<FP>();
    G.T = fp_mul(G.X, G.Y);
    return ok;
}
// sum_j k_j * G_j for one row.  k: the row's `count` scalars; tables: the set's combs; rw: the lane's nine recoded words, word w
// at rw[w * stride], rewritten by every term.  A lane without a row (`valid` false) computes on row 0's scalars with top = -1.
// Every term runs from the ROW'S OWN top digit, not from the wave's: an addition of the cached identity rescales the running
// sum (by 4 Z), so a trip count taken over the wave would make a row's limbs depend on the rows beside it.
ZC_DI pt gens_row_sum(const u64* __restrict__ k, int count, const u32* __restrict__ tables, u32* __restrict__ rw, int stride, bool valid)
{
    pt Q = pt_identity();
#pragma unroll 1
    for (int j = 0; j < count; j++) {
        u64 l[5];
        load_scalar(l, k + 5 * j);
        int top = scalar_recode256(rw, stride, l);
        if (!valid) top = -1;
        Q = base_mul_onto(Q, tables + (size_t)j * GENS_TABLE_WORDS, rw, stride, top);
    }
    return Q;
}

}  // namespace zc

// the kernels: hipcc only (the host emulation of the test tier builds the device functions above with a C++ compiler)
#if defined(__HIPCC__)
#include "zc_kernels.hip.h"

namespace zc {

// One workgroup of 128 lanes per generator; lane e builds column e of table blockIdx.x.  bad[j] (zeroed by the host) is set
// where generator j is no point of the curve; its table is then left unwritten.  The verdict is the same in every lane.
ZC_KERNEL void k_gens_table_build(const u64* points, u32* tables, u32* bad)
{
    const int e = threadIdx.x, j = blockIdx.x;
    if (e >= ZC_BASE_ENTRIES) return;
    pt G;
    if (!gens_normalise(G, points + 20 * j)) {
        if (e == 0) bad[j] = 1;
        return;
    }
    comb_table_column(tables + (size_t)j * GENS_TABLE_WORDS, G, e);
}
// One row per lane.  The lane's recoded words sit in its own LDS column (9 x ZC_BLOCK words, 9 KB per workgroup whatever
// `count` is); no lane reads another lane's column, so there is no barrier.
ZC_KERNEL void k_ed_mul_gens(const u64* k, u64* out, const u32* tables, u32 count, size_t n)
{
    __shared__ u32 srw[9 * ZC_BLOCK];
    const size_t i = gid();
    const bool valid = i < n;
    const pt Q = gens_row_sum(k + 5 * count * (valid ? i : 0), (int)count, tables, srw + threadIdx.x, ZC_BLOCK, valid);
    if (valid) pt_store(out + 20 * i, Q);
}
ZC_KERNEL void k_ris_mul_gens_compress(const u64* k, uint8_t* out, const u32* tables, u32 count, size_t n)
{
    __shared__ u32 srw[9 * ZC_BLOCK];
    const size_t i = gid();
    const bool valid = i < n;
    const pt Q = gens_row_sum(k + 5 * count * (valid ? i : 0), (int)count, tables, srw + threadIdx.x, ZC_BLOCK, valid);
    u64 w[4];
    fe_to_words256(w, ris_compress(Q));
    if (valid) store_words256(out + 32 * i, w);
}

}  // namespace zc
#endif
