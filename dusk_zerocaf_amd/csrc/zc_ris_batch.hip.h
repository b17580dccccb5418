// zc_ris_batch.hip.h -- batched Ristretto calls whose rows share work: zc_ris_double_and_compress (below) and
// zc_ris_lincomb_sum (further down: the weighted sum of all rows as one MSM).
//
// out = RistrettoPoint(2 P).compress(): the reference's Double (edwards.rs:579-592) followed by compress
// (ristretto.rs:398-425), without the square root.  compress pays one (p-5)/8 power per row (about 250 squarings, 265
// multiplications in all) that nothing can share.  The encoding of a DOUBLED point needs only the inverse of a product, and
// Montgomery's trick shares one inversion among the rows of a lane.  With d = EDWARDS_D, for a row (X : Y : Z : T):
//     e = 2 X Y    f = Z^2 + d T^2    g = Y^2 + X^2    h = Z^2 - d T^2         (2P = (e f : g h : f h : e g), a = -1)
//     w = (e g) (f h)                   the one value to invert
//     Zinv = (e g) / w = 1 / (f h)      Tinv = (f h) / w = 1 / (e g)
//     magic = INV_SQRT_A_MINUS_D
//     if !is_positive(e g Zinv): (e, g, h, magic) = (g, -e, f SQRT_MINUS_ONE, SQRT_MINUS_ONE)
//     if !is_positive(h e Zinv): g = -g
//     s = (h - g) magic g Tinv;  out = to_bytes(|s|)
// Every quantity a decision reads has degree 0 in the coordinates, so any representative of the point gives the same bytes.
// The two negations only change the sign of g, and |s| is taken last: with g' the unsigned choice (e or g) and tau the product
// of the two signs, |s| = |(h - tau g') g' magic Tinv| -- a subtraction or an addition, no negated value is ever formed.
//
// Multiplications per row (squarings counted as multiplications): the terms 6 (X Y, X^2, Y^2, Z^2, T^2, d T^2), e g, f h and
// w 3: 9 in either pass (the limbs are used as they come: no conversion into the Montgomery domain).  Forward pass 9 + 1
// (running product) = 10; backward pass 9 + 2 (peel the inverse, step it) + 2 (Zinv, Tinv) + 1 (first sign) + 1 (f i) + 2
// (second sign) + 3 (s) = 20; three leaves of the domain for the sign tests and two for the zero test, half a
// multiplication each.  About 32 per row plus 1 / c of a division-step inversion (about 45), against about 265 for
// ris_compress after a doubling's 9.  (A wave that holds a coordinate of 1.5 * 2^252 or more pays 8 more.)
//
// Zero by value: w = 0 mod p exactly for the points of E[8] (e g = 0: X Y = 0 or X^2 + Y^2 = 0) and for Z = 0, T = 0 garbage;
// the reference's composition returns 32 zero bytes for E[8].  Such a row takes the neutral value in the shared product, gets
// 32 zero bytes, and changes nothing in its lane (the rule of fe_invert_chunk and ed_to_affine_chunk).  Rows off the curve get
// bytes that depend on their own words only; every launch form decides by canonical values, so the forms agree byte for byte.
#pragma once
#include "zc_curve.hip.h"
#include "zc_msm_plan.h"      // ZC_BLOCK

namespace zc {

struct ris_dc_terms {
    fe e, f, g, h;       // e, f, g lazy (limbs < 2^30), h normalized and below 8N
    fe eg, fh, w;        // R-class
    bool zero;           // w = 0 mod p
};

template <bool ILP>
ZC_DI fe ris_dc_mul(const fe& x, const fe& y) { return ILP ? mont_mul_ilp<FP>(x, y) : mont_mul<FP>(x, y); }
template <bool ILP>
ZC_DI fe ris_dc_sqr(const fe& x) { return ILP ? mont_sqr_ilp<FP>(x) : mont_sqr<FP>(x); }

// e, f, g, h and their products from the four coordinates X, Y, Z, T as residues with one common factor, each below 3N
// (ris_dc_load's limbs below 1.5 N; a point in registers, R-class: products of operands below 3N stay below 1.02 N, their sums
// below 2.04 N as the comments of ris_dc_finish want them)
template <bool ILP>
ZC_DI ris_dc_terms ris_dc_terms_of(const fe (&c)[4])
{
    ris_dc_terms t;
    const fe xy = ris_dc_mul<ILP>(c[0], c[1]);
    const fe zz = ris_dc_sqr<ILP>(c[2]);
    const fe dtt = ris_dc_mul<ILP>(fe_const<FP>(ModP::D_M), ris_dc_sqr<ILP>(c[3]));
    t.e = fe_add(xy, xy);
    t.g = fe_add(ris_dc_sqr<ILP>(c[1]), ris_dc_sqr<ILP>(c[0]));
    t.f = fe_add(zz, dtt);
    t.h = fp_sub(zz, dtt);
    t.eg = ris_dc_mul<ILP>(t.e, t.g);
    t.fh = ris_dc_mul<ILP>(t.f, t.h);
    t.w = ris_dc_mul<ILP>(t.eg, t.fh);
    t.zero = fp_is_zero(t.w);
    return t;
}
// ... for the record at `row` (twenty words, any: a word's bits from 2^52 up are not read)
template <bool ILP>
ZC_DI ris_dc_terms ris_dc_load(const u64* __restrict__ row)
{
    // The plain limbs serve as Montgomery residues (of X / R ...: one common factor, and the encoding does not depend on the
    // representative).  The bounds below want operands under 1.5 N: a top limb below 1.5 * 2^44, as every canonical value
    // has.  Anything larger is reduced first (x (R mod N) / R = x, below 1.5 N) -- by the whole wave, so that honest batches
    // never diverge; the residue is the same either way, and nothing below depends on more than the residue.
    fe c[4];
    bool big = false;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        u64 l[5];
        load5(l, row + 5 * k);
        c[k] = fe_from_limbs52(l);
        big |= ((l[4] & M52) >> 43) >= 3;
    }
    if (wave_any(big)) {
#pragma unroll
        for (int k = 0; k < 4; k++) c[k] = ris_dc_mul<ILP>(c[k], fe_one_m<FP>());
    }
    return ris_dc_terms_of<ILP>(c);
}

// The row's 32 bytes as four words from its terms and winv = 1 / w (Montgomery form, R-class); zeros for a row with w = 0.
template <bool ILP>
ZC_DI void ris_dc_finish(u64 (&out)[4], const ris_dc_terms& t, const fe& winv)
{
    const fe zinv = ris_dc_mul<ILP>(t.eg, winv);
    const fe tinv = ris_dc_mul<ILP>(t.fh, winv);
    const bool rotate = !fp_is_positive(ris_dc_mul<ILP>(t.eg, zinv));
    fe e = t.e, g = t.g;
    fe_carry(e);                                                             // sums of two products of operands below 1.5 N: below 2.02 N,
    fe_carry(g);                                                             // R-class once the limbs are normalized
    const fe e2 = fe_select(rotate, g, e);
    const fe g2 = fe_select(rotate, e, g);                                   // unsigned: the sign is (rotate ? -1 : +1)
    const fe h2 = fe_select(rotate, ris_dc_mul<ILP>(t.f, fe_const<FP>(ModP::SQRT_M1_M)), t.h);
    const fe magic = fe_select(rotate, fe_const<FP>(ModP::SQRT_M1_M), fe_const<FP>(ModP::INV_SQRT_A_MINUS_D_M));
    const bool negate = !fp_is_positive(ris_dc_mul<ILP>(h2, ris_dc_mul<ILP>(e2, zinv)));
    const fe diff = fe_select(rotate != negate, fe_add(h2, g2), fp_sub(h2, g2));       // h - tau g'
    const fe s = ris_dc_mul<ILP>(ris_dc_mul<ILP>(ris_dc_mul<ILP>(diff, magic), g2), tinv);
    const fe sc = fp_canon(s);
    fe_to_words256(out, fe_select(fe_is_positive_canon<FP>(sc), sc, fe_n_minus_canon<FP>(sc)));
    if (t.zero) out[0] = out[1] = out[2] = out[3] = 0;
}

// One row on its own: one inversion (k_ris_double_compress, small batches).
ZC_DI void ris_double_compress_row(u64 (&out)[4], const u64* __restrict__ row)
{
    const ris_dc_terms t = ris_dc_load<false>(row);
    ris_dc_finish<false>(out, t, fp_invert(t.w));                            // 0 -> 0, and the row's bytes are zeroed
}
// The same for a point that is in registers already (Montgomery form, R-class coordinates): the bytes of 2 Q (zc_shared.hip.h)
template <bool ILP>
ZC_DI void ris_double_compress_pt(u64 (&out)[4], const pt& Q)
{
    const fe c[4] = {Q.X, Q.Y, Q.Z, Q.T};
    const ris_dc_terms t = ris_dc_terms_of<ILP>(c);
    ris_dc_finish<ILP>(out, t, fp_invert(t.w));
}

// One lane's share of the batch: Montgomery's trick over w of the up to `c` rows lo, lo + stride, ... (as ed_to_affine_chunk:
// stride = number of lanes, so that the lanes of a wave touch neighbouring records in both passes).  The forward pass forms
// w_j and parks the running product of the rows before j; one inversion; the backward pass forms the row's terms again from its
// record, peels 1 / w_j off the running inverse and finishes the row.
//
// Where the prefix products wait: the call may write nothing but its 32-byte output rows, and the nine-word register form
// the other chunked kernels park does not fit one.  So the prefix is made canonical (two conditional subtractions: it is
// below 3N) and parked as a 256-bit integer in the row's OWN output bytes, which the backward pass replaces with the encoding.
// The load in the backward pass must be issued by the lane that stored, with the same address: a lane's own global stores
// and loads to one address stay in program order, nothing orders them against another lane's without a fence.  Both passes
// derive the address from (lo, stride, j) alone, and `out32` must not overlap `p` (the record is read again after the store).
template <bool ILP = false>
ZC_DI void ris_double_compress_chunk(const u64* p, uint8_t* out32, size_t n, size_t lo, size_t stride, int c)
{
    const size_t avail = (n - lo + stride - 1) / stride;
    const int cnt = (int)(avail < (size_t)c ? avail : (size_t)c);
    const fe neutral = fe_one_m<FP>();
    fe acc = neutral;
    for (int j = 0; j < cnt; j++) {
        const size_t i = lo + (size_t)j * stride;
        const ris_dc_terms t = ris_dc_load<ILP>(p + 20 * i);
        u64 park[4];
        fe_to_words256(park, fe_cond_sub_n<FP>(fe_cond_sub_n<FP>(acc)));     // the product of the rows before j, times R
        u64* slot = reinterpret_cast<u64*>(out32 + 32 * i);                  // 32-byte records, 8-byte aligned
#pragma unroll
        for (int k = 0; k < 4; k++) slot[k] = park[k];
        acc = ris_dc_mul<ILP>(acc, fe_select(t.zero, neutral, t.w));
    }
    // plain inverse of the register value, times R^3: inv pre / R = R / w_j, the Montgomery form of 1 / w_j, from here on
    fe inv = ris_dc_mul<ILP>(fp_inverse_of_register(acc), fe_const<FP>(ModP::R3));
    for (int j = cnt - 1; j >= 0; j--) {
        const size_t i = lo + (size_t)j * stride;
        const ris_dc_terms t = ris_dc_load<ILP>(p + 20 * i);
        u64* slot = reinterpret_cast<u64*>(out32 + 32 * i);
        u64 park[4];
#pragma unroll
        for (int k = 0; k < 4; k++) park[k] = slot[k];                       // this lane's own store of the forward pass
        const fe winv = ris_dc_mul<ILP>(inv, fe_from_words256(park));
        inv = ris_dc_mul<ILP>(inv, fe_select(t.zero, neutral, t.w));
        ris_dc_finish<ILP>(park, t, winv);
#pragma unroll
        for (int k = 0; k < 4; k++) slot[k] = park[k];
    }
}

// ---------------------------------------------------------------- zc_ris_lincomb_sum: one MSM over all rows, from bytes
// out = compress(b B + sum_{i, ok_i} sum_j w_ij decompress(E_ij)): three passes prepare ordinary MSM inputs -- 160-byte point
// records and canonical 40-byte scalars in a workspace of the device slot -- and the MSM pipeline runs on them as it stands.
//   k_ris_sum_prepare   one lane per (row, term): decode (one inverse-square-root power, bound by the multiplier), the record
//                       (the identity for an undecodable encoding), w_ij = val(z_i) val(k_ij) mod L, one decode flag
//   k_ris_sum_rows      one lane per row: ok_i = the AND of the row's flags; a rejected row's scalars become zero (the MSM's
//                       contract: a zero scalar contributes the identity whatever the record holds); t_i = ok_i ? z_i kB_i : 0
//   k_sc_sum            b = sum_i t_i mod L: strided partial sums per lane, a tree in LDS per workgroup, one partial per
//                       workgroup, a second launch of one workgroup over the partials
// Every scalar and weight is read BY VALUE (sc_muladd_limbs52: val(w) = sum (w_i mod 2^52) 2^(52 i), reduced mod L), so what
// the MSM receives is canonical and both of its regimes multiply by exactly w_ij.  Addition mod L is associative and every
// partial is canonical: b does not depend on the launch geometry.
constexpr size_t SC_SUM_ROWS_PER_LANE = 4;      // first launch of k_sc_sum: a workgroup covers ZC_BLOCK * SC_SUM_ROWS_PER_LANE rows ...
constexpr size_t SC_SUM_MAX_BLOCKS = 1024;      // ... until this many workgroups; beyond, the lanes stride further

// val(a) val(z) mod L, canonical (z null: val(a) mod L)
ZC_DI void ris_sum_weighted(u64 (&r)[5], const u64* __restrict__ a, const u64* __restrict__ z)
{
    u64 x[5], y[5] = {1, 0, 0, 0, 0};
    const u64 zero[5] = {0, 0, 0, 0, 0};
    load5(x, a);
    if (z) load5(y, z);
    sc_muladd_limbs52(r, x, y, zero);
}
// One (row, term) pair: the encoding's four words -> record, weighted scalar, decode flag.
ZC_DI void ris_sum_pair(const u64 (&enc)[4], const u64* __restrict__ k, const u64* __restrict__ z, u64* __restrict__ point,
                        u64* __restrict__ scalar, uint8_t* __restrict__ flag)
{
    pt P;
    const bool dec = ris_decompress(P, enc);
    pt_store(point, pt_select(dec, P, pt_identity()));
    u64 w[5];
    ris_sum_weighted(w, k, z);
    store5(scalar, w);
    *flag = dec ? 1 : 0;
}
// One row: `flags` and `scalars` are the row's `terms` entries of the workspace; ok and t may be null (t: no base term).
ZC_DI void ris_sum_row(const uint8_t* __restrict__ flags, size_t terms, u64* __restrict__ scalars, const u64* __restrict__ kb,
                       const u64* __restrict__ z, uint8_t* __restrict__ ok, u64* __restrict__ t)
{
    bool all = true;
    for (size_t j = 0; j < terms; j++) all &= flags[j] != 0;
    const u64 zero[5] = {0, 0, 0, 0, 0};
    if (!all)
        for (size_t j = 0; j < terms; j++) store5(scalars + 5 * j, zero);
    if (ok) *ok = all ? 1 : 0;
    if (t) {
        u64 w[5];
        ris_sum_weighted(w, kb, z);                                          // by every lane: the multiplier's path is chosen per wave
#pragma unroll
        for (int i = 0; i < 5; i++) w[i] = all ? w[i] : 0;
        store5(t, w);
    }
}
// the record of the base term's pair: RISTRETTO_BASEPOINT, Z = 1
ZC_DI void ris_sum_store_basepoint(u64* __restrict__ o)
{
    pt B;
    B.X = fe_const<FP>(ModP::BASE_X_M);
    B.Y = fe_const<FP>(ModP::BASE_Y_M);
    B.Z = fe_one_m<FP>();
    B.T = fe_const<FP>(ModP::BASE_T_M);
    pt_store(o, B);
}
// a + b mod L for canonical a, b
ZC_DI fe sc_add_canon(const fe& a, const fe& b)
{
    fe s = fe_add(a, b);
    fe_carry(s);
    return fe_cond_sub_n<ModL>(s);                                           // below 2L
}
// lane g of `lanes`: t[g] + t[g + lanes] + ... mod L over n canonical scalars
ZC_DI fe sc_sum_strided(const u64* __restrict__ t, size_t n, size_t g, size_t lanes)
{
    fe acc = fe_zero();
    for (size_t i = g; i < n; i += lanes) {
        u64 l[5];
        load5(l, t + 5 * i);
        acc = sc_add_canon(acc, fe_from_limbs52(l));
    }
    return acc;
}
// one level of a workgroup's tree over its lanes' partials: lane `lane` < half takes its partner's (barriers between the levels)
ZC_DI void sc_sum_tree_step(fe* part, int lane, int half) { part[lane] = sc_add_canon(part[lane], part[lane + half]); }
ZC_DI void sc_sum_store(u64* __restrict__ out, const fe& s)
{
    u64 l[5];
    fe_to_limbs52(l, s);
    store5(out, l);
}

}  // namespace zc

// the kernels: hipcc only (the host emulation of the test tier builds the device functions above with a C++ compiler)
#if defined(__HIPCC__)
#include "zc_kernels.hip.h"

namespace zc {

// one row per lane, one inversion each: batches too small to share
ZC_KERNEL void k_ris_double_compress(const u64* p, uint8_t* out32, size_t n)
{
    const size_t i = gid();
    if (i >= n) return;
    u64 w[4];
    ris_double_compress_row(w, p + 20 * i);
    u64* o = reinterpret_cast<u64*>(out32 + 32 * i);
#pragma unroll
    for (int k = 0; k < 4; k++) o[k] = w[k];
}
// `c` rows per lane share one inversion (ris_double_compress_chunk)
ZC_KERNEL void k_ris_double_compress_chunked(const u64* p, uint8_t* out32, size_t n, int c)
{
    const size_t lanes = (n + (size_t)c - 1) / (size_t)c, g = gid();
    if (g < lanes) ris_double_compress_chunk<false>(p, out32, n, g, lanes, c);
}
// the same for launches of at most one wave per SIMD, on the independent-chain multiplier
ZC_KERNEL void k_ris_double_compress_chunked_lone(const u64* p, uint8_t* out32, size_t n, int c)
{
    const size_t lanes = (n + (size_t)c - 1) / (size_t)c, g = gid();
    if (g < lanes) ris_double_compress_chunk<true>(p, out32, n, g, lanes, c);
}

// zc_ris_lincomb_sum (see above).  One lane per (row, term): in32, k as zc_ris_lincomb lays them out; z null = no weights.
ZC_KERNEL void k_ris_sum_prepare(const uint8_t* in32, const u64* k, const u64* z, u64* points, u64* scalars, uint8_t* flags, size_t terms, size_t pairs)
{
    const size_t g = gid();
    if (g >= pairs) return;
    u64 w[4];
    load_words256(w, in32 + 32 * g);
    ris_sum_pair(w, k + 5 * g, z ? z + 5 * (g / terms) : nullptr, points + 20 * g, scalars + 5 * g, flags + g);
}
// one lane per row; ok null when not requested; kb, t and base_record (the base term's record, written by lane 0) null without a base term
ZC_KERNEL void k_ris_sum_rows(const uint8_t* flags, u64* scalars, const u64* kb, const u64* z, uint8_t* ok, u64* t, u64* base_record, size_t terms, size_t n)
{
    const size_t i = gid();
    if (i >= n) return;
    if (i == 0 && base_record) ris_sum_store_basepoint(base_record);
    ris_sum_row(flags + terms * i, terms, scalars + 5 * terms * i, kb ? kb + 5 * i : nullptr, z ? z + 5 * i : nullptr, ok ? ok + i : nullptr,
                t ? t + 5 * i : nullptr);
}
// out[workgroup] = the sum mod L of the canonical scalars t[g], t[g + lanes], ... of the workgroup's lanes
ZC_KERNEL void k_sc_sum(const u64* t, size_t n, u64* out)
{
    __shared__ fe part[ZC_BLOCK];
    const int lane = threadIdx.x;
    part[lane] = sc_sum_strided(t, n, gid(), (size_t)gridDim.x * ZC_BLOCK);
    __syncthreads();
    for (int half = ZC_BLOCK / 2; half > 0; half >>= 1) {
        if (lane < half) sc_sum_tree_step(part, lane, half);
        __syncthreads();
    }
    if (lane == 0) sc_sum_store(out + 5 * (size_t)blockIdx.x, part[0]);
}

}  // namespace zc
#endif
