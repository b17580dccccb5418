// shared_scalar_plan_emul.cpp -- TEST-ONLY driver of zc_shared_scalar.h (what zc_ed_scalar_mul_shared / zc_ris_mul_shared do with
// their one scalar on the host), beside the device's own rule for the effective scalar (zc_curve.hip.h: scalar_effective) built
// for the host.  Never shipped.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "../../dusk_zerocaf_amd/csrc/zc_curve.hip.h"
#include "../../dusk_zerocaf_amd/csrc/zc_shared_scalar.h"

extern "C" void zc_bound_fail(const char* what, int line)
{
    std::fprintf(stderr, "zc_arith.hip.h:%d: bound violated: %s\n", line, what);
    std::abort();
}

constexpr int SHARED_PLAN_WORDS = 5 + 5 + 5 + 2 * (2 + 2 * zc::SHARED_MAX_STEPS);      // what emul_shared_plan writes

extern "C" {
// out: k_eff by the host's rule (5 limbs), k_eff by the device's rule (5 limbs), k' (5 limbs), then for the schedule of k_eff and
// for the schedule of k': steps, tail, and 53 x (doublings, digit) -- unused steps zero.  Every entry a 64-bit integer.
void emul_shared_plan(const uint64_t* k, int64_t* out)
{
    uint64_t host[5], dev[5], half[5];
    zc::shared_effective(host, k);
    for (int j = 0; j < 5; j++) dev[j] = k[j];
    zc::scalar_effective(dev);
    zc::shared_to_limbs52(half, zc::shared_half_mod_l(zc::shared_from_limbs52(host)));
    for (int j = 0; j < 5; j++) {
        out[j] = (int64_t)host[j];
        out[5 + j] = (int64_t)dev[j];
        out[10 + j] = (int64_t)half[j];
    }
    const zc::shared_schedule s[2] = {zc::shared_schedule_ed(k), zc::shared_schedule_wire(k)};
    int64_t* o = out + 15;
    for (int f = 0; f < 2; f++) {
        *o++ = s[f].steps;
        *o++ = s[f].tail;
        for (int i = 0; i < zc::SHARED_MAX_STEPS; i++) {
            const bool used = (uint32_t)i < s[f].steps;
            *o++ = used ? (int64_t)zc::shared_step_doublings(s[f].step[i]) : 0;
            *o++ = used ? (int64_t)zc::shared_step_digit(s[f].step[i]) : 0;
        }
    }
}
int emul_shared_plan_words() { return SHARED_PLAN_WORDS; }
}
