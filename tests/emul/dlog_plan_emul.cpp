// dlog_plan_emul.cpp -- TEST-ONLY: dusk_zerocaf_amd/csrc/zc_dlog_plan.h behind a C interface, built with g++ alone (no HIP header
// anywhere).  Never shipped.
#include "../../dusk_zerocaf_amd/csrc/zc_dlog_plan.h"

using namespace zc;

extern "C" {
// min_bits, max_bits, max_steps, chunk, steps_per_launch, max_launches, block, record_bytes, setup_stride, setup_w, setup_words
void plan_dlog_constants(unsigned long long* out)
{
    const unsigned long long c[] = {DLOG_MIN_BITS, DLOG_MAX_BITS, DLOG_MAX_STEPS, (unsigned long long)DLOG_CHUNK, DLOG_STEPS_PER_LAUNCH, DLOG_MAX_LAUNCHES,
                                    (unsigned long long)DLOG_BLOCK, DLOG_RECORD_BYTES, (unsigned long long)DLOG_SETUP_STRIDE, (unsigned long long)DLOG_SETUP_W, DLOG_SETUP_WORDS};
    for (int i = 0; i < 11; i++) out[i] = c[i];
}
// records, slots, table bytes, builder lanes
void plan_dlog_sizes(unsigned t, unsigned long long* out)
{
    out[0] = dlog_records(t);
    out[1] = dlog_slots(t);
    out[2] = dlog_table_bytes(t);
    out[3] = dlog_build_lanes(t);
}
int plan_dlog_bits_ok(unsigned t) { return dlog_bits_ok(t); }
int plan_dlog_bound_ok(unsigned long long bound, unsigned t) { return dlog_bound_ok(bound, t); }
unsigned long long plan_dlog_steps(unsigned long long bound, unsigned t) { return dlog_steps(bound, t); }
unsigned long long plan_dlog_launches(unsigned long long bound, unsigned t) { return dlog_launches(bound, t); }
// first, steps, chunks of launch k
void plan_dlog_slice(unsigned long long bound, unsigned t, unsigned long long k, unsigned long long* out)
{
    const DlogSlice s = dlog_slice(bound, t, k);
    out[0] = s.first;
    out[1] = s.steps;
    out[2] = s.chunks;
}
unsigned long long plan_dlog_offset_word(unsigned long long k) { return dlog_offset_word(k); }
unsigned long long plan_dlog_home(unsigned long long w0, unsigned t) { return dlog_home(w0, t); }
unsigned plan_dlog_tag(unsigned long long w0) { return dlog_tag(w0); }
long plan_dlog_build_slots(unsigned long long* slots, unsigned t, const unsigned long long* records)
{
    return dlog_build_slots(reinterpret_cast<uint64_t*>(slots), t, reinterpret_cast<const uint64_t*>(records));
}
long plan_dlog_find(const unsigned long long* slots, unsigned t, const unsigned long long* records, const unsigned long long* rec)
{
    return dlog_find(reinterpret_cast<const uint64_t*>(slots), t, reinterpret_cast<const uint64_t*>(records), reinterpret_cast<const uint64_t*>(rec));
}
}
