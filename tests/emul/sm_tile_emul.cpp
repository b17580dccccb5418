// sm_tile_emul.cpp -- TEST-ONLY host build of the persistent strict kernel's tile loop (k_ed_scalar_mul_pw).
// emul.cpp treats a wave as one element, which cannot exercise a ballot-driven schedule; here a tile is 64 real
// lanes, every ballot is a loop over them, and the per-lane functions are the very ones the kernel calls
// (zc_curve.hip.h: sm_lane, sm_g_step, sm_d_step, pt_doubling_identities_hold, ptm_double_valid).  Never shipped.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "../../dusk_zerocaf_amd/csrc/zc_curve.hip.h"

extern "C" void zc_bound_fail(const char* what, int line)
{
    std::fprintf(stderr, "zc_arith.hip.h:%d: bound violated: %s\n", line, what);
    std::abort();
}

using namespace zc;

namespace {
constexpr int WAVE = 64;
struct stash_host {
    fe c[4];
    fe get(int i) const { return c[i]; }
    void put(int i, const fe& x) { c[i] = x; }
};
struct lane_regs {
    bool valid;
    u32 sk[9];
    ptm N, Q;
    stash_host S;
    sm_lane L;
};
template <class PRED>
bool wave_any_of(const lane_regs (&w)[WAVE], PRED pred)
{
    bool r = false;
    for (int j = 0; j < WAVE; j++) r = r || pred(w[j]);
    return r;
}
}

// Tiles of 64 consecutive rows, the last one ragged (lanes past n run with nbits = 0 on row 0's data, as in the kernel).
// steps: per tile {generic steps, doubling steps, 1 if the gate let doubling steps run}.  allow_d = 0 switches doubling
// steps off for every tile (the schedule of ZC_SCHED=unified).
extern "C" void emul_sm_tiles(const u64* p, const u64* k, u64* out, size_t n, int* steps, int allow_d)
{
    static lane_regs w[WAVE];
    const size_t ntiles = (n + WAVE - 1) / WAVE;
    for (size_t t = 0; t < ntiles; t++) {
        bool d_ok = allow_d != 0;
        for (int j = 0; j < WAVE; j++) {
            lane_regs& r = w[j];
            const size_t i = t * WAVE + (size_t)j;
            r.valid = i < n;
            const size_t own = r.valid ? i : 0;
            u64 l[5];
            load_scalar(l, k + 5 * own);
            int nbits;
            scalar_to_words(r.sk, 1, l, nbits);
            const pt P = pt_load(p + 20 * own);
            r.N = ptm_from_pt(P);
            r.Q = ptm_from_pt(pt_identity());
            if (r.valid && !pt_doubling_identities_hold(P, r.N)) d_ok = false;
            r.L = sm_lane_init(r.sk, r.valid ? nbits : 0);
        }
        int g = 0, d = 0;
        while (wave_any_of(w, [](const lane_regs& r) { return r.L.active; })) {
            for (int j = 0; j < WAVE; j++) sm_g_step(w[j].L, w[j].N, w[j].Q, w[j].S, w[j].sk, 1);
            g++;
            const bool any_active = wave_any_of(w, [](const lane_regs& r) { return r.L.active; });
            const bool any_at_top = wave_any_of(w, [](const lane_regs& r) { return sm_at_top(r.L); });
            if (d_ok && sm_tile_wants_d_step(any_active, any_at_top)) {
                for (int j = 0; j < WAVE; j++) sm_d_step(w[j].L, w[j].N, w[j].S, w[j].sk, 1);
                d++;
            }
        }
        for (int j = 0; j < WAVE; j++)
            if (w[j].valid) pt_store(out + 20 * (t * WAVE + (size_t)j), ptm_to_pt(w[j].Q));
        steps[3 * t] = g;
        steps[3 * t + 1] = d;
        steps[3 * t + 2] = d_ok ? 1 : 0;
    }
}
