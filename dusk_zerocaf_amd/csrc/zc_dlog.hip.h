// zc_dlog.hip.h -- bounded discrete logs: m with P = m * G, 0 <= m < bound, by baby steps and giant steps (zerocaf_hip_dlog.h).
//
// A table holds the records of j * G_eff, j < 2^t (G_eff = G, or 4 G for equality modulo E[4]), filed in an open-addressing slot
// array (zc_dlog_plan.h), the stride S = -2^t * G_eff and the offsets W_k = k * 1024 * S as cached affine points.  A row walks
// Q_g = Q_0 + g * S and looks every Q_g up.  The record of a point is its canonical affine y with the parity of canonical x in
// bit 255: injective on curve points with Z != 0, and -- unlike ed_compress, whose sign is the root's -- free of a square root.
//
// The inversion behind y = Y / Z is shared by the DLOG_CHUNK steps of a chunk, inside the lane (a row can poison nobody else):
//   forward   per step  Q + S mixed addition                                   7 multiplications
//                       U = Y a, a = a Z  (a: product of the Z so far)          2
//   once      I = 1 / a                                                         one division-step inversion
//   backward  per step  y = U I, I = I Z                                        2
// 11 multiplications per giant step + inversion / DLOG_CHUNK.  U and Z wait in the lane's LDS column: 18 words per step.  The
// search never works out x: the neighbouring giant step tells +j from -j (dlog_search).  The record builder runs the same two
// halves over runs of consecutive multiples, with V = X a as a third field for the parity bit.
//
// Nothing here is constant-time.  The device functions compile for the host (tests/emul/dlog_emul.cpp).
#pragma once
#include "zc_curve.hip.h"
#include "zc_dlog_plan.h"

namespace zc {

// A cached affine point (Z = 1) as it travels in kernel arguments and in the setup block.
struct dlog_step {
    fe ymx, ypx, t2d;
};
constexpr int DLOG_STAGE_WORDS = 18 * DLOG_CHUNK;          // a lane's staged fields in the search
constexpr int DLOG_BUILD_STAGE_WORDS = 27 * DLOG_CHUNK;    // and in the record builder

ZC_DI niels dlog_niels(const dlog_step& s)
{
    niels q;
    q.ymx = s.ymx;
    q.ypx = s.ypx;
    q.z = fe_one_m<FP>();
    q.t2d = s.t2d;
    return q;
}
ZC_DI void dlog_put(u32* __restrict__ o, int stride, int slot, const fe& a)
{
#pragma unroll
    for (int w = 0; w < 9; w++) o[(size_t)(9 * slot + w) * stride] = a.v[w];
}
ZC_DI fe dlog_get(const u32* __restrict__ o, int stride, int slot)
{
    fe a;
#pragma unroll
    for (int w = 0; w < 9; w++) a.v[w] = o[(size_t)(9 * slot + w) * stride];
    return a;
}
ZC_DI void dlog_step_store(u32* __restrict__ o, const dlog_step& s)
{
    dlog_put(o, 1, 0, s.ymx);
    dlog_put(o, 1, 1, s.ypx);
    dlog_put(o, 1, 2, s.t2d);
}
ZC_DI dlog_step dlog_step_load(const u32* __restrict__ o)
{
    dlog_step s;
    s.ymx = dlog_get(o, 1, 0);
    s.ypx = dlog_get(o, 1, 1);
    s.t2d = dlog_get(o, 1, 2);
    return s;
}
// (X/Z, Y/Z, 1, XY/Z^2) of a point with Z != 0
ZC_DI pt dlog_affine(const pt& P)
{
    const fe zi = fp_invert(P.Z);
    pt G;
    G.X = fp_mul(P.X, zi);
    G.Y = fp_mul(P.Y, zi);
    G.Z = fe_one_m<FP>();
    G.T = fp_mul(G.X, G.Y);
    return G;
}
ZC_DI dlog_step dlog_step_of(const pt& affine)
{
    const niels q = niels_from_pt(affine);
    dlog_step s;
    s.ymx = q.ymx;
    s.ypx = q.ypx;
    s.t2d = q.t2d;
    return s;
}
ZC_DI bool dlog_is_identity(const pt& P) { return fp_is_zero(P.X) && fp_eq(P.Y, P.Z); }

// What a table keeps beside its records, from the caller's point p (20 limbs; T is not read): the verdict, and where that is
// DLOG_SETUP_OK the records of the setup block at `out`.  One lane.
ZC_DI u32 dlog_setup(u32* __restrict__ out, const u64* __restrict__ p, unsigned t, unsigned flags)
{
    pt P;
    P.X = fe_load_mont<FP>(p);
    P.Y = fe_load_mont<FP>(p + 5);
    P.Z = fe_load_mont<FP>(p + 10);
    if (!ed_is_valid(P) || fp_is_zero(P.Z)) return DLOG_SETUP_NOT_A_POINT;     // Z = 0 by value: it passes the projective equation when X Y = 0
    pt G = dlog_affine(P);
    if (flags & DLOG_FLAG_COSET4) {
        G = pt_add(G, G);
        G = dlog_affine(pt_add(G, G));
    }
    pt E = G;
#pragma unroll 1
    for (int i = 0; i < 3; i++) E = pt_add(E, E);
    if (dlog_is_identity(E)) return DLOG_SETUP_SMALL_ORDER;                      // G_eff in E[8]: its order is no multiple of L
    dlog_step_store(out + DLOG_SETUP_STRIDE * DLOG_SETUP_G, dlog_step_of(G));
    pt S = G;
#pragma unroll 1
    for (unsigned i = 0; i < t; i++) S = pt_add(S, S);
    S = pt_neg(dlog_affine(S));
    dlog_step_store(out + DLOG_SETUP_STRIDE * DLOG_SETUP_S, dlog_step_of(S));
    pt L = S;                                                                     // DLOG_STEPS_PER_LAUNCH * S
#pragma unroll 1
    for (uint64_t i = 1; i < DLOG_STEPS_PER_LAUNCH; i *= 2) L = pt_add(L, L);
    pt W = pt_identity();
#pragma unroll 1
    for (int k = 0; k < (int)DLOG_MAX_LAUNCHES; k++) {
        dlog_step_store(out + DLOG_SETUP_STRIDE * (DLOG_SETUP_W + k), dlog_step_of(dlog_affine(W)));
        W = pt_add(W, L);
    }
    return DLOG_SETUP_OK;
}

// The forward half of a chunk: stages U_i = Y_i a_i, Z_i and -- WITH_X -- V_i = X_i a_i of Q + i * S, i < DLOG_CHUNK, with
// a_i = Z_0 .. Z_(i-1); leaves Q + DLOG_CHUNK * S in Q and returns 1 / (Z_0 .. Z_(DLOG_CHUNK-1)).  Complete additions on curve
// points: no Z is zero.  A step takes 2 (3 WITH_X) fields of 9 words in the lane's column.
template <bool WITH_X>
ZC_DI fe dlog_chunk_forward(pt& Q, const niels& S, u32* __restrict__ stage, int stride)
{
    constexpr int F = WITH_X ? 3 : 2;
    fe a = fe_one_m<FP>();
#pragma unroll 1
    for (int i = 0; i < DLOG_CHUNK; i++) {
        dlog_put(stage, stride, F * i, fp_mul(Q.Y, a));
        dlog_put(stage, stride, F * i + 1, Q.Z);
        if (WITH_X) dlog_put(stage, stride, F * i + 2, fp_mul(Q.X, a));
        a = fp_mul(a, Q.Z);
        Q = pt_add_cached<false, true>(Q, S);
    }
    return fp_invert(a);
}
// Step i of the backward half, I = 1 / (Z_0 .. Z_i) on entry and 1 / (Z_0 .. Z_(i-1)) on return: canonical y as four words.
template <bool WITH_X>
ZC_DI void dlog_chunk_y(u64 (&w)[4], const fe& I, const u32* __restrict__ stage, int stride, int i)
{
    fe_to_words256(w, fp_canon(fp_mul(dlog_get(stage, stride, (WITH_X ? 3 : 2) * i), I)));
}
ZC_DI u64 dlog_chunk_x_parity(const fe& I, const u32* __restrict__ stage, int stride, int i)
{
    return fp_canon(fp_mul(dlog_get(stage, stride, 3 * i + 2), I)).v[0] & 1u;
}
template <bool WITH_X>
ZC_DI fe dlog_chunk_back(const fe& I, const u32* __restrict__ stage, int stride, int i) { return fp_mul(I, dlog_get(stage, stride, (WITH_X ? 3 : 2) * i + 1)); }

// One lane of the record builder: the records of j * G_eff, j = lane * DLOG_BUILD_RUN + i, i < DLOG_BUILD_RUN.  The start multiple
// by double-and-add over the t bits a lane index has, then the run as one chunk.
ZC_DI void dlog_build_run(u64* __restrict__ records, const u32* __restrict__ setup, unsigned t, size_t lane, u32* __restrict__ stage, int stride)
{
    const niels G = dlog_niels(dlog_step_load(setup + DLOG_SETUP_STRIDE * DLOG_SETUP_G));
    const size_t first = lane * (size_t)DLOG_BUILD_RUN;
    pt Q = pt_identity();
#pragma unroll 1
    for (int b = (int)t - 1; b >= 0; b--) {
        Q = pt_add(Q, Q);
        Q = pt_select(((first >> b) & 1) != 0, pt_add_cached<false, true>(Q, G), Q);
    }
    fe I = dlog_chunk_forward<true>(Q, G, stage, stride);
#pragma unroll 1
    for (int i = DLOG_BUILD_RUN - 1; i >= 0; i--) {
        u64 w[4];
        dlog_chunk_y<true>(w, I, stage, stride, i);
        w[3] |= dlog_chunk_x_parity(I, stage, stride, i) << 63;
        I = dlog_chunk_back<true>(I, stage, stride, i);
#pragma unroll
        for (int k = 0; k < 4; k++) records[4 * (first + (size_t)i) + k] = w[k];
    }
}

// A table as the search reads it.
struct dlog_table {
    const u64* records;
    const u64* slots;
    u32 t;
};
// The j whose record holds the y in w, or -1.  Two records never share a y: j G = -j' G would make (j + j') G the identity.
ZC_DI long dlog_lookup(const dlog_table& T, const u64 (&w)[4])
{
    const u32 tag = dlog_tag(w[0]);
    long hit = -1;
    for (size_t s = dlog_home(w[0], T.t);; s = dlog_next(s, T.t)) {
        const u64 slot = T.slots[s];
        if (slot == DLOG_EMPTY) break;
        if (dlog_slot_tag(slot) != tag) continue;
        const u64* rec = T.records + 4 * (size_t)dlog_slot_index(slot);
        if (rec[0] == w[0] && rec[1] == w[1] && rec[2] == w[2] && (rec[3] & ~DLOG_PARITY_BIT) == w[3]) hit = (long)dlog_slot_index(slot);
    }
    return hit;
}
// Is w the y of record j?
ZC_DI bool dlog_y_is(const dlog_table& T, const u64 (&w)[4], size_t j)
{
    const u64* rec = T.records + 4 * j;
    return rec[0] == w[0] && rec[1] == w[1] && rec[2] == w[2] && (rec[3] & ~DLOG_PARITY_BIT) == w[3];
}
// The row's start: T from X, Y and Z (the caller's is not trusted: (X Z, Y Z, Z^2, X Y) is the same point), two doublings for a
// table of 4 G, then the launch's offset.
ZC_DI pt dlog_start(const pt& P, bool coset4, const niels& W)
{
    pt Q;
    Q.X = fp_mul(P.X, P.Z);
    Q.Y = fp_mul(P.Y, P.Z);
    Q.Z = fp_sqr(P.Z);
    Q.T = fp_mul(P.X, P.Y);
    if (coset4) {
        Q = pt_add(Q, Q);
        Q = pt_add(Q, Q);
    }
    return pt_add_cached<false, true>(Q, W);
}
// `chunks` chunks from Q = Q_first: true and m = g * 2^t + j for the giant step g = first + ... whose point is j * G_eff, if
// m < bound.  A lane that is not `live` (no row, a row that is no curve point, a row found by an earlier launch) walks along
// on whatever it holds and reports nothing; the walk ends when every lane of the wave is through.
//
// THE SIGN WITHOUT x.  y(Q_g) = y(j G_eff) leaves Q_g = +-j G_eff, and the record's parity bit would settle it at the price of a
// third staged field (X a) per step.  The neighbouring giant step settles it for nothing: with T = 2^t and 0 < j < T,
//   Q_g = +j G_eff  =>  Q_(g+1) = Q_g - T G_eff = -(T - j) G_eff: its y IS record T - j's;   Q_(g-1) = (T + j) G_eff: it is NOT
//   Q_g = -j G_eff  =>  Q_(g+1) = -(T + j) G_eff: NOT;                                        Q_(g-1) = (T - j) G_eff: it IS
// ("is not": (T + j) = +-(T - j) modulo the order of G_eff, a multiple of L, would need 2 j = 0 or 2 T = 0).  A chunk is walked
// from its last step down, so y of step i + 1 is at hand for every step but the chunk's last, whose verdict waits for y of the
// step before it.  j = 0 is the identity: no sign.  Two staged fields per step keep a wave's LDS at 18 KB: two waves per SIMD.
ZC_DI bool dlog_search(u64& m_out, pt Q, const dlog_table& T, const niels& S, u64 first, u64 chunks, u64 bound, bool live, u32* __restrict__ stage, int stride)
{
    static_assert(DLOG_CHUNK >= 2, "the last step of a chunk is judged by the step before it");
    const size_t size = dlog_records(T.t);
    bool found = false;
#pragma unroll 1
    for (u64 c = 0; c < chunks; c++) {
        if (wave_all(found || !live)) break;
        fe I = dlog_chunk_forward<false>(Q, S, stage, stride);
        u64 above[4] = {0, 0, 0, 0};         // y of step i + 1
        long waiting = -1;                  // the chunk's last step matched record `waiting` (> 0) in y
#pragma unroll 1
        for (int i = DLOG_CHUNK - 1; i >= 0; i--) {
            if (live && !found) {
                u64 w[4];
                dlog_chunk_y<false>(w, I, stage, stride, i);
                long j = -1;                // the record step `at` is known to be, sign included
                int at = i;
                if (waiting > 0 && !dlog_y_is(T, w, size - (size_t)waiting)) {
                    j = waiting;
                    at = DLOG_CHUNK - 1;
                }
                waiting = -1;
                const long hit = j < 0 ? dlog_lookup(T, w) : -1;
                if (hit == 0) j = 0;
                else if (hit > 0 && i == DLOG_CHUNK - 1) waiting = hit;
                else if (hit > 0 && dlog_y_is(T, above, size - (size_t)hit)) j = hit;
                const u64 m = ((first + c * DLOG_CHUNK + (u64)at) << T.t) + (u64)(j < 0 ? 0 : j);
                if (j >= 0 && m < bound) {
                    found = true;
                    m_out = m;
                }
#pragma unroll
                for (int k = 0; k < 4; k++) above[k] = w[k];
            }
            I = dlog_chunk_back<false>(I, stage, stride, i);
        }
    }
    return found;
}
// A row of limbs: false where it is no point of the curve by value (P then holds no point).
ZC_DI bool dlog_load_ed(pt& P, const u64* __restrict__ p)
{
    P = pt_load(p);
    return ed_is_valid(P) && !fp_is_zero(P.Z);
}

}  // namespace zc

// the kernels: hipcc only (the host emulation of the test tier builds the device functions above with a C++ compiler)
#if defined(__HIPCC__)
#include "zc_kernels.hip.h"

namespace zc {

#define ZC_KERNEL_DLOG extern "C" __global__ __launch_bounds__(DLOG_BLOCK)

// What one launch of the search is told (kernel arguments: the two cached points sit in scalar registers).
struct dlog_launch {
    dlog_table table;
    u32 coset4;
    u32 launch;          // k: launch 0 writes the defaults, later ones skip rows that were found
    u64 first;           // first giant step = k * DLOG_STEPS_PER_LAUNCH
    u64 chunks;
    u64 bound;
    dlog_step S, W;      // the stride and W_k
};

ZC_KERNEL_DLOG void k_dlog_setup(const u64* point, u32* setup, u32 t, u32 flags)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) setup[0] = dlog_setup(setup, point, t, flags);
}
ZC_KERNEL_DLOG void k_dlog_records(const u32* setup, u64* records, u32 t)
{
    __shared__ u32 stage[DLOG_BUILD_STAGE_WORDS * DLOG_BLOCK];
    const size_t lane = (size_t)blockIdx.x * DLOG_BLOCK + threadIdx.x;
    if (lane >= dlog_build_lanes(t)) return;               // no barrier below: a lane reads its own column only
    dlog_build_run(records, setup, t, lane, stage + threadIdx.x, DLOG_BLOCK);
}
template <class LOAD>
ZC_DI void dlog_rows(LOAD load, u64* m_out, uint8_t* found, uint8_t* ok, const dlog_launch& A, size_t n)
{
    __shared__ u32 stage[DLOG_STAGE_WORDS * DLOG_BLOCK];
    const size_t i = (size_t)blockIdx.x * DLOG_BLOCK + threadIdx.x;
    const bool valid = i < n;
    pt P;
    const bool good = load(P, valid ? i : 0);
    bool live = valid && good;
    if (A.launch == 0) {
        if (valid) {
            m_out[i] = 0;
            found[i] = 0;
            if (ok) ok[i] = good ? 1 : 0;
        }
    } else if (valid && found[i]) {
        live = false;
    }
    P = pt_select(good, P, pt_identity());
    const pt Q = dlog_start(P, A.coset4 != 0, dlog_niels(A.W));
    u64 m = 0;
    if (dlog_search(m, Q, A.table, dlog_niels(A.S), A.first, A.chunks, A.bound, live, stage + threadIdx.x, DLOG_BLOCK)) {
        m_out[i] = m;
        found[i] = 1;
    }
}
ZC_KERNEL_DLOG void k_ed_dlog(const u64* p, u64* m_out, uint8_t* found, uint8_t* ok, dlog_launch A, size_t n)
{
    dlog_rows([&](pt& P, size_t i) { return dlog_load_ed(P, p + 20 * i); }, m_out, found, ok, A, n);
}
ZC_KERNEL_DLOG void k_ris_dlog(const uint8_t* in, u64* m_out, uint8_t* found, uint8_t* ok, dlog_launch A, size_t n)
{
    dlog_rows([&](pt& P, size_t i) {
        u64 w[4];
        load_words256(w, in + 32 * i);
        return ris_decompress(P, w);
    }, m_out, found, ok, A, n);
}

}  // namespace zc
#endif
