// sm_g_step_emul.cpp -- TEST-ONLY host build of ONE lane's generic steps (zc_curve.hip.h: sm_g_step), checked step by step
// for what a step must leave alone: an addition keeps N, a doubling keeps Q, and a lane that is not active keeps Q, N and
// its whole state -- the step has no early return, the lane's inactivity is folded into its commit predicates.  Never shipped.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../dusk_zerocaf_amd/csrc/zc_curve.hip.h"

extern "C" void zc_bound_fail(const char* what, int line)
{
    std::fprintf(stderr, "zc_arith.hip.h:%d: bound violated: %s\n", line, what);
    std::abort();
}

using namespace zc;

namespace {
struct stash_host {
    fe c[4];
    fe get(int i) const { return c[i]; }
    void put(int i, const fe& x) { c[i] = x; }
};
bool same(const ptm& a, const ptm& b) { return std::memcmp(&a, &b, sizeof(ptm)) == 0; }
bool same(const sm_lane& a, const sm_lane& b)
{
    return a.pos == b.pos && a.nbits == b.nbits && a.cur == b.cur && a.taken == b.taken && a.has_stash == b.has_stash && a.active == b.active;
}
}

// Runs the lane of (p, k) as a tile of its own -- generic steps, with use_d != 0 (valid points only) alternating with doubling
// steps as the kernel does, so that additions come from the stash too -- and, before the first step and after every generic
// step, a copy of the lane with `active` cleared through one more generic step.  Returns the number of violated checks;
// out = Q as the kernel stores it, steps[0] = generic steps run, steps[1] = checks made.
extern "C" int emul_g_step_keeps(const u64* p, const u64* k, u64* out, int* steps, int use_d)
{
    u32 sk[9];
    u64 l[5];
    load_scalar(l, k);
    int nbits;
    scalar_to_words(sk, 1, l, nbits);
    const pt P = pt_load(p);
    ptm N = ptm_from_pt(P), Q = ptm_from_pt(pt_identity());
    stash_host S;
    std::memset(&S, 0xA5, sizeof S);                      // never selected without has_stash: any pattern will do
    sm_lane L = sm_lane_init(sk, nbits);
    int bad = 0, g = 0, checks = 0;
    auto frozen_step_keeps_all = [&]() {
        sm_lane L2 = L;
        ptm N2 = N, Q2 = Q;
        L2.active = false;
        const sm_lane L0 = L2;
        sm_g_step(L2, N2, Q2, S, sk, 1);
        checks++;
        if (!same(N2, N) || !same(Q2, Q) || !same(L2, L0)) bad++;
    };
    frozen_step_keeps_all();                              // inactive from the first step (and the only check for nbits == 0)
    while (L.active) {
        const bool add = L.has_stash || sm_bit_pending(L);
        const ptm N0 = N, Q0 = Q;
        const sm_lane L0 = L;
        sm_g_step(L, N, Q, S, sk, 1);
        g++;
        checks++;
        const bool kept = add ? same(N, N0) && L.pos == L0.pos && !L.has_stash && (L0.has_stash ? L.taken == L0.taken : L.taken)
                              : same(Q, Q0) && L.pos == L0.pos + 1 && !L.taken && !L.has_stash;
        if (!kept) bad++;
        frozen_step_keeps_all();                          // retired mid-way: after every step, whatever the state
        if (use_d && sm_tile_wants_d_step(L.active, sm_at_top(L))) {
            sm_d_step(L, N, S, sk, 1);
            frozen_step_keeps_all();                      // ... with an addend waiting in the stash too
        }
    }
    pt_store(out, ptm_to_pt(Q));
    steps[0] = g;
    steps[1] = checks;
    return bad;
}
