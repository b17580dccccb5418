// shared_lincomb_plan_emul.cpp -- TEST-ONLY driver of the joint schedule of zc_shared_scalar.h (what zc_ed_lincomb_shared /
// zc_ris_lincomb_shared do with their scalar vector on the host), beside the single-scalar schedules it must agree with for
// one term.  g++ alone, no HIP include.  Never shipped.
#include <cstddef>
#include <cstdint>
#include "../../dusk_zerocaf_amd/csrc/zc_shared_scalar.h"

constexpr int LINCOMB_PLAN_FORM_WORDS = 3 + zc::SHARED_LINCOMB_MAX_TERMS + 3 * zc::SHARED_LINCOMB_MAX_STEPS;
constexpr int LINCOMB_PLAN_WORDS = 2 * LINCOMB_PLAN_FORM_WORDS;      // what emul_shared_lincomb_plan writes

extern "C" {
// out, for the schedule of the k_eff,j and then for the schedule of the k'_j: steps, tail, terms, the eight entry counts, and
// 424 x (doublings, digit, term) -- unused steps zero.  Every entry a 64-bit integer.
void emul_shared_lincomb_plan(const uint64_t* k, size_t terms, int64_t* out)
{
    const zc::shared_lincomb_schedule s[2] = {zc::shared_lincomb_schedule_ed(k, terms), zc::shared_lincomb_schedule_wire(k, terms)};
    int64_t* o = out;
    for (int f = 0; f < 2; f++) {
        *o++ = s[f].steps;
        *o++ = s[f].tail;
        *o++ = s[f].terms;
        for (int j = 0; j < zc::SHARED_LINCOMB_MAX_TERMS; j++) *o++ = s[f].entries[j];
        for (int i = 0; i < zc::SHARED_LINCOMB_MAX_STEPS; i++) {
            const bool used = (uint32_t)i < s[f].steps;
            *o++ = used ? (int64_t)zc::shared_step_doublings(s[f].step[i]) : 0;
            *o++ = used ? (int64_t)zc::shared_step_digit(s[f].step[i]) : 0;
            *o++ = used ? (int64_t)zc::shared_step_term(s[f].step[i]) : 0;
        }
    }
}
// the single-scalar schedules of one scalar, in the layout above without the term column: steps, tail, 53 x (doublings, digit)
void emul_shared_single_plan(const uint64_t* k, int64_t* out)
{
    const zc::shared_schedule s[2] = {zc::shared_schedule_ed(k), zc::shared_schedule_wire(k)};
    int64_t* o = out;
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
int emul_shared_lincomb_plan_words() { return LINCOMB_PLAN_WORDS; }
int emul_shared_lincomb_schedule_bytes() { return (int)sizeof(zc::shared_lincomb_schedule); }
}
