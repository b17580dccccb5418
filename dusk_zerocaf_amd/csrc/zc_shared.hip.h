// zc_shared.hip.h -- ONE scalar applied to a whole batch: zc_ed_scalar_mul_shared and zc_ris_mul_shared (zerocaf_hip_ext_shared.h).
//
// The windowed core of scalar_mul_fast (zc_curve.hip.h) recodes a scalar per lane into LDS, adds the cached identity for a
// zero digit because the lanes' digits differ, and the wire form ends in ris_compress's (p-5)/8 power.  With one scalar for
// the batch the digit schedule is wave-uniform by construction, so it is a width-5 signed SLIDING window: the host recodes
// the scalar once (zc_shared_scalar.h) and the schedule travels by value in the kernel arguments -- no LDS, no per-lane digit,
// no identity addition, T computed only by the doubling in front of an addition.
//   table     {1, 3, ..., 15} P in cached form, eight 128-byte records in the lane's 1 KB of the wave's ring slot: one
//             doubling with T for 2P, seven cached additions of 2P, eight conversions: 73 multiplications
//   step      r dedicated doublings (7 each, 8 for the last), one cached addition (8) of the record |d| >> 1, negated by
//             a wave-uniform branch for d < 0
// A 252-bit scalar has about 252 / 6 = 42 non-zero digits: about 252 * 7 + 43 * 9 + 73 = 2 224 multiplications per row
// against the 2 394 of scalar_mul_fast.
// The wire form multiplies by k' = (k mod L) / 2 mod L and leaves through the double-and-encode formula of zc_ris_batch.hip.h on
// the point in registers: encode(2 (k' P)) = encode(k P + m L P) for an integer m, and for a decoded P (which lies in 2 E) the
// point m L P is one of E[4], which the encoding does not see.  One division-step inversion per lane instead of the
// square-root power: about 2 520 multiplications per row against about 2 910.
//
// Like scalar_mul_fast, NOT the reference's formula sequence: the same group element as double_and_add's k P, a different
// projective representative, deterministic limbs that depend on the row and the scalar only.
#pragma once
#include "zc_ris_batch.hip.h"
#include "zc_shared_scalar.h"

namespace zc {

// table[j] = (2 j + 1) P, cached form.  Two live points: the running multiple and the cached 2 P.
template <class TABLE>
ZC_DI void shared_table_build(const pt& P, const TABLE table)
{
    niels_store(table.entry(0), niels_from_pt(P));
    const niels c2 = niels_from_pt(pt_double_fast<true>(P));
    pt q = P;
#pragma unroll 1
    for (int j = 1; j < 8; j++) {
        q = pt_add_cached(q, c2);
        niels_store(table.entry(j), niels_from_pt(q));
    }
}
template <bool ILP>
ZC_DI pt shared_doublings(pt Q, u32 r)                    // r doublings, T from the last one only
{
    for (; r > 1; r--) Q = pt_double_fast<false, ILP>(Q);
    if (r) Q = pt_double_fast<true, ILP>(Q);
    return Q;
}
// The additions of the schedule, from the top digit down; the doublings after the last one are shared_tail's, so that a
// kernel can give its table slot back in between.  Every value read from `s` is wave-uniform.
template <bool ILP, class TABLE>
ZC_DI pt shared_steps(const TABLE table, const shared_schedule& s)
{
    pt Q = pt_identity();
    for (u32 i = 0; i < s.steps; i++) {
        const u32 w = s.step[i];
        Q = shared_doublings<ILP>(Q, shared_step_doublings(w));
        const int d = shared_step_digit(w);
        niels c = niels_load(table.entry((d < 0 ? -d : d) >> 1));
        if (d < 0) {                                      // -c: swap (Y - X, Y + X), negate 2dT (niels_cond_neg, decided per wave)
            const fe ymx = c.ymx;
            c.ymx = c.ypx;
            c.ypx = ymx;
            c.t2d = fe_neg_lazy<FP>(c.t2d);
        }
        Q = pt_add_cached<ILP>(Q, c);
    }
    return Q;
}
template <bool ILP>
ZC_DI pt shared_tail(const pt& Q, const shared_schedule& s) { return shared_doublings<ILP>(Q, s.tail); }

// The Edwards form of one row, as the kernel runs it (small launches on the independent-chain multiplier).
template <class TABLE>
ZC_DI pt shared_mul_steps(const pt& P, const TABLE table, const shared_schedule& s)
{
    shared_table_build(P, table);
    return zc_small_launch() ? shared_steps<true>(table, s) : shared_steps<false>(table, s);
}
ZC_DI pt shared_mul_tail(const pt& Q, const shared_schedule& s)
{
    return zc_small_launch() ? shared_tail<true>(Q, s) : shared_tail<false>(Q, s);
}
// The wire form of one row: `s` is the schedule of k'.  Returns the accept flag; an undecodable row walks the schedule as the
// identity (its lanes take part in the wave's uniform control flow) and leaves as 32 zero bytes.
ZC_DI bool shared_ris_decode(pt& P, const u64 (&w)[4])
{
    pt D;
    const bool dec = ris_decompress(D, w);
    P = pt_select(dec, D, pt_identity());
    return dec;
}
ZC_DI void shared_ris_encode(u64 (&w)[4], const pt& Q, bool dec)
{
    ris_double_compress_pt<false>(w, Q);                  // zeros for a shared factor of 0 mod p: the identity's (and E[8]'s) way out
    if (!dec) w[0] = w[1] = w[2] = w[3] = 0;
}

// ---------------------------------------------------------------- a scalar VECTOR for the batch: out[i] = sum_j k_j P_ij
// zc_ed_lincomb_shared / zc_ris_lincomb_shared.  The host merges the terms' recodings into one schedule (zc_shared_scalar.h:
// shared_lincomb_schedule): one doubling chain and one cached addition per non-zero digit of ANY term, about 252 * 7 +
// 43.5 * 10 t multiplications per row against the 1 827 + 567 t of lincomb_fast with its per-lane digits.  Term j's table
// {1, 3, .., 15} P_ij lies in unit j of the wave's slot (`tables.term(j)`), built only as far as the schedule reads it.

// table[j] = (2 j + 1) P for j < entries (wave-uniform): shared_table_build cut short.  entries = 1 (k_j = +-2^e, the
// coefficient 1 of an ElGamal decryption) costs one conversion, entries = 0 (k_j = 0) nothing.  The records are
// shared_table_build's own whatever the bound, so one term gives the limbs of the single-scalar call.
template <class TABLE>
ZC_DI void shared_table_build_upto(const pt& P, const TABLE table, u32 entries)
{
    if (entries == 0) return;
    niels_store(table.entry(0), niels_from_pt(P));
    if (entries == 1) return;
    const niels c2 = niels_from_pt(pt_double_fast<true>(P));
    pt q = P;
#pragma unroll 1
    for (u32 j = 1; j < entries; j++) {
        q = pt_add_cached(q, c2);
        niels_store(table.entry((int)j), niels_from_pt(q));
    }
}
// shared_steps with a term index.  A step without doublings (two terms with a digit at one position) takes T from the
// addition before it: pt_add_cached returns all four coordinates.
template <bool ILP, class TABLES>
ZC_DI pt shared_lincomb_steps(const TABLES tables, const shared_lincomb_schedule& s)
{
    pt Q = pt_identity();
    for (u32 i = 0; i < s.steps; i++) {
        const u32 w = s.step[i];
        Q = shared_doublings<ILP>(Q, shared_step_doublings(w));
        const int d = shared_step_digit(w);
        niels c = niels_load(tables.term((int)shared_step_term(w)).entry((d < 0 ? -d : d) >> 1));
        if (d < 0) {                                      // -c, decided per wave (see shared_steps)
            const fe ymx = c.ymx;
            c.ymx = c.ypx;
            c.ypx = ymx;
            c.t2d = fe_neg_lazy<FP>(c.t2d);
        }
        Q = pt_add_cached<ILP>(Q, c);
    }
    return Q;
}
template <class TABLES>
ZC_DI pt shared_lincomb_sum(const TABLES tables, const shared_lincomb_schedule& s)
{
    return zc_small_launch() ? shared_lincomb_steps<true>(tables, s) : shared_lincomb_steps<false>(tables, s);
}
ZC_DI pt shared_lincomb_tail(const pt& Q, const shared_lincomb_schedule& s)
{
    return zc_small_launch() ? shared_doublings<true>(Q, s.tail) : shared_doublings<false>(Q, s.tail);
}
// The wire form's terms, as ris_lincomb_decode / ris_lincomb_table (zc_curve.hip.h) handle them: a decoded point (Z = 1)
// waits as X | Y | T in the first record of its own table, which the build then overwrites.  An undecodable term is parked
// as the identity, so its lane walks the schedule with curve points; the row leaves as zero bytes.
template <class TABLE>
ZC_DI bool shared_lincomb_decode(const u64 (&w)[4], const TABLE table)
{
    pt P;
    const bool dec = shared_ris_decode(P, w);
    u32* e = table.entry(0);
#pragma unroll
    for (int k = 0; k < 9; k++) {
        e[k] = P.X.v[k];
        e[9 + k] = P.Y.v[k];
        e[18 + k] = P.T.v[k];
    }
    return dec;
}
template <class TABLE>
ZC_DI void shared_lincomb_table(const TABLE table, u32 entries)
{
    pt P;
    const u32* e = table.entry(0);
#pragma unroll
    for (int k = 0; k < 9; k++) {
        P.X.v[k] = e[k];
        P.Y.v[k] = e[9 + k];
        P.T.v[k] = e[18 + k];
    }
    P.Z = fe_one_m<FP>();
    shared_table_build_upto(P, table, entries);
}

}  // namespace zc

// the kernels: hipcc only (the host emulation of the test tier builds the device functions above with a C++ compiler)
#if defined(__HIPCC__)
#include "zc_kernels.hip.h"

namespace zc {

// One row per lane.  The ring slot is taken and given back as in k_ed_scalar_mul_fast; apart from the ring's `hold` word the
// kernel uses no LDS.  The row's number is formed afresh from the wave's number (a scalar register since the first
// instruction) and v_mbcnt wherever it is needed, so nothing derived from threadIdx.x stays live across the loop.
ZC_KERNEL_3W void k_ed_scalar_mul_shared(const u64* p, const shared_schedule sched, u64* out, u32* table, u32* ring, u32 ring_slots, u32 n)
{
    const u32 wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const u32 wave_first = blockIdx.x * ZC_BLOCK + wave_in_block * 64u;
    __shared__ u32 hold[ZC_BLOCK / 64];
    const ring_table mine = ring_acquire(table, ring, hold + wave_in_block, ring_slots);
    if (!mine.base) {                                      // the wave gave up waiting for its table slot (wave-uniform): poison, no barrier follows
        const u32 i = wave_first + lane_id_fresh();
        if (i < n)
            for (int j = 0; j < 20; j++) out[20 * (size_t)i + j] = ~(u64)0;
        return;
    }
    const u32 row = wave_first + lane_id_fresh();
    pt Q = shared_mul_steps(pt_load(p + 20 * (size_t)(row < n ? row : 0)), mine, sched);
    ring_release(ring, hold + wave_in_block);              // the last table read is behind us
    Q = shared_mul_tail(Q, sched);
    const u32 i_late = wave_first + lane_id_fresh();
    if (i_late < n) pt_store(out + 20 * (size_t)i_late, Q);
}
// bytes in, bytes out: decode, the same loop over the schedule of k', double-and-encode of the result in registers
ZC_KERNEL_3W void k_ris_mul_shared(const uint8_t* in, const shared_schedule sched, uint8_t* out, uint8_t* ok, u32* table, u32* ring, u32 ring_slots, u32 n)
{
    const u32 wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const u32 wave_first = blockIdx.x * ZC_BLOCK + wave_in_block * 64u;
    u64 w[4];
    pt P;
    {
        const u32 row = wave_first + lane_id_fresh();
        load_words256(w, in + 32 * (size_t)(row < n ? row : 0));
    }
    const bool dec = shared_ris_decode(P, w);
    __shared__ u32 hold[ZC_BLOCK / 64];                    // the table slot is held for the multiplication only
    const ring_table mine = ring_acquire(table, ring, hold + wave_in_block, ring_slots);
    if (!mine.base) {                                      // the wave gave up waiting for its table slot (wave-uniform): poison, no barrier follows
        const u32 i = wave_first + lane_id_fresh();
        if (i < n) {
            w[0] = w[1] = w[2] = w[3] = ~(u64)0;
            store_words256(out + 32 * (size_t)i, w);
            if (ok) ok[i] = 0;
        }
        return;
    }
    pt Q = shared_mul_steps(P, mine, sched);
    ring_release(ring, hold + wave_in_block);
    Q = shared_mul_tail(Q, sched);
    shared_ris_encode(w, Q, dec);
    const u32 i_late = wave_first + lane_id_fresh();
    if (i_late < n) {
        store_words256(out + 32 * (size_t)i_late, w);
        if (ok) ok[i_late] = dec ? 1 : 0;
    }
}

// ---- a scalar vector for the batch: out[i] = sum_j k_j P_ij (zc_ed_lincomb_shared, zc_ris_lincomb_shared) ----------
// One row per lane; the wave's slot is sched.terms consecutive units of the ring, re-based as k_ed_lincomb does it
// (ring_table_terms).  No LDS beyond the ring's `hold` words at any term count -- the digits are the schedule's, in scalar
// registers -- so the workgroup has 256 lanes throughout.  The slot goes back after the last addition; the tail doublings
// need no table.
ZC_KERNEL_3W void k_ed_lincomb_shared(const u64* p, const shared_lincomb_schedule sched, u64* out, u32* table, u32* ring, u32 ring_slots, u32 units_per_xcd,
                                      u32 n)
{
    const u32 wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const u32 wave_first = blockIdx.x * ZC_BLOCK + wave_in_block * 64u;
    __shared__ u32 hold[ZC_BLOCK / 64];
    const ring_table got = ring_acquire(table, ring, hold + wave_in_block, ring_slots);
    if (!got.base) {                                       // the wave gave up waiting for its table slot (wave-uniform): poison, no barrier follows
        const u32 i = wave_first + lane_id_fresh();
        if (i < n)
            for (int j = 0; j < 20; j++) out[20 * (size_t)i + j] = ~(u64)0;
        return;
    }
    const u32 terms = sched.terms;
    const u32 named = (u32)((size_t)(got.base - table) / (64 * 256));          // xcc * RING_SLOTS + slot (wave-uniform)
    const u32 xcc = named / RING_SLOTS, slot = named % RING_SLOTS;
    const ring_table_terms mine{table + (size_t)(xcc * units_per_xcd + slot * terms) * (64 * 256)};
#pragma unroll 1
    for (u32 j = 0; j < terms; j++) {
        const u32 row = wave_first + lane_id_fresh();
        const u32 entries = sched.entries[j];              // wave-uniform: a term the schedule never reads is not even loaded
        if (entries) shared_table_build_upto(pt_load(p + 20 * ((size_t)(row < n ? row : 0) * terms + j)), mine.term((int)j), entries);
    }
    pt Q = shared_lincomb_sum(mine, sched);
    ring_release(ring, hold + wave_in_block);              // the last table read is behind us
    Q = shared_lincomb_tail(Q, sched);
    const u32 i_late = wave_first + lane_id_fresh();
    if (i_late < n) pt_store(out + 20 * (size_t)i_late, Q);
}
// bytes in, bytes out over the schedule of the k'_j.  Decoding and table building are two `unroll 1` loops for the reason
// given above k_ris_lincomb (zc_kernels.hip.h); a term under a zero scalar builds nothing but is decoded, for the accept flag.
ZC_KERNEL_3W void k_ris_lincomb_shared(const uint8_t* in, const shared_lincomb_schedule sched, uint8_t* out, uint8_t* ok, u32* table, u32* ring, u32 ring_slots,
                                       u32 units_per_xcd, u32 n)
{
    const u32 wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const u32 wave_first = blockIdx.x * ZC_BLOCK + wave_in_block * 64u;
    __shared__ u32 hold[ZC_BLOCK / 64];
    const ring_table got = ring_acquire(table, ring, hold + wave_in_block, ring_slots);
    if (!got.base) {                                       // the wave gave up waiting for its table slot (wave-uniform): poison, no barrier follows
        const u32 i = wave_first + lane_id_fresh();
        if (i < n) {
            const u64 ones[4] = {~(u64)0, ~(u64)0, ~(u64)0, ~(u64)0};
            store_words256(out + 32 * (size_t)i, ones);
            if (ok) ok[i] = 0;
        }
        return;
    }
    const u32 terms = sched.terms;
    const u32 named = (u32)((size_t)(got.base - table) / (64 * 256));          // xcc * RING_SLOTS + slot (wave-uniform)
    const u32 xcc = named / RING_SLOTS, slot = named % RING_SLOTS;
    const ring_table_terms mine{table + (size_t)(xcc * units_per_xcd + slot * terms) * (64 * 256)};
    bool dec = true;                                       // the only per-lane value that survives a decode
#pragma unroll 1
    for (u32 j = 0; j < terms; j++) {
        const u32 row = wave_first + lane_id_fresh();
        u64 w[4];
        load_words256(w, in + 32 * ((size_t)(row < n ? row : 0) * terms + j));
        dec = shared_lincomb_decode(w, mine.term((int)j)) && dec;
    }
#pragma unroll 1
    for (u32 j = 0; j < terms; j++) shared_lincomb_table(mine.term((int)j), sched.entries[j]);
    pt Q = shared_lincomb_sum(mine, sched);
    ring_release(ring, hold + wave_in_block);
    Q = shared_lincomb_tail(Q, sched);
    u64 w[4];
    shared_ris_encode(w, Q, dec);
    const u32 i_late = wave_first + lane_id_fresh();
    if (i_late < n) {
        store_words256(out + 32 * (size_t)i_late, w);
        if (ok) ok[i_late] = dec ? 1 : 0;
    }
}

}  // namespace zc
#endif
