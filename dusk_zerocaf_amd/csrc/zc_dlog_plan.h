// zc_dlog_plan.h -- what the bounded discrete logs (zerocaf_hip.hip: zc_dlog_create, zc_ed_dlog, zc_ris_dlog; kernels in
// zc_dlog.hip.h) derive from (table_bits, bound) before they touch the device, and the one piece of the table that is built on the
// host: the slot array.  Plain C++17 without any HIP include: tests/test_dlog_plan_emul.py drives it on the CPU.  No knob reads
// into it.  The hash and the slot format are constexpr, so the kernels use the very functions the host inserts with.
#pragma once
#include <cstddef>
#include <cstdint>

namespace zc {

constexpr unsigned DLOG_MIN_BITS = 4;                      // ZC_DLOG_MIN_BITS
constexpr unsigned DLOG_MAX_BITS = 22;                     // ZC_DLOG_MAX_BITS
constexpr uint64_t DLOG_MAX_STEPS = 65536;                 // ZC_DLOG_MAX_STEPS: giant steps per call
constexpr unsigned DLOG_FLAG_COSET4 = 1u;                  // ZC_DLOG_COSET4
// Giant steps that share one inversion (a lane stages 2 x DLOG_CHUNK fields of 9 words: zc_dlog.hip.h).  A compile-time choice;
// `python -m dusk_zerocaf_amd.build --variant NAME ZC_DLOG_CHUNK=8` builds an A/B library, the product carries no switch.
#ifndef ZC_DLOG_CHUNK
#define ZC_DLOG_CHUNK 4
#endif
constexpr int DLOG_CHUNK = ZC_DLOG_CHUNK;
constexpr uint64_t DLOG_STEPS_PER_LAUNCH = 1024;           // no launch walks more giant steps than this
constexpr uint64_t DLOG_MAX_LAUNCHES = DLOG_MAX_STEPS / DLOG_STEPS_PER_LAUNCH;     // 64: the offsets W_k a table holds
constexpr int DLOG_BLOCK = 64;                             // lanes of a workgroup of the search and the record builder: one wave
constexpr int DLOG_BUILD_RUN = DLOG_CHUNK;                 // records one lane of the builder makes (one inversion per lane)
constexpr size_t DLOG_RECORD_BYTES = 32;                   // canonical y, the parity of canonical x in bit 255
constexpr uint64_t DLOG_EMPTY = ~(uint64_t)0;              // a slot that holds nothing
constexpr uint64_t DLOG_PARITY_BIT = (uint64_t)1 << 63;    // of word 3 of a record
static_assert(DLOG_STEPS_PER_LAUNCH % DLOG_CHUNK == 0, "a launch is a whole number of chunks");
static_assert(((size_t)1 << DLOG_MIN_BITS) >= (size_t)DLOG_BUILD_RUN, "the smallest table is at least one builder lane");

// ---- sizes
constexpr size_t dlog_records(unsigned t) { return (size_t)1 << t; }
constexpr size_t dlog_slots(unsigned t) { return (size_t)2 << t; }                 // load factor one half: a probe sequence always ends
constexpr size_t dlog_record_bytes(unsigned t) { return dlog_records(t) * DLOG_RECORD_BYTES; }
constexpr size_t dlog_slot_bytes(unsigned t) { return dlog_slots(t) * sizeof(uint64_t); }
constexpr size_t dlog_table_bytes(unsigned t) { return dlog_record_bytes(t) + dlog_slot_bytes(t); }    // per device slot
constexpr size_t dlog_build_lanes(unsigned t) { return dlog_records(t) / (size_t)DLOG_BUILD_RUN; }

// ---- the hash: a record is filed under its low word w0 (bits 0..63 of canonical y).  h = w0 * 2^64 / phi; the slot is the top
// t + 1 bits of h, the tag its low 32 bits.  A slot is tag << 32 | j (j < 2^22, so never DLOG_EMPTY).
constexpr uint64_t dlog_mix(uint64_t w0) { return w0 * 0x9E3779B97F4A7C15ull; }
constexpr size_t dlog_home(uint64_t w0, unsigned t) { return (size_t)(dlog_mix(w0) >> (63 - t)); }
constexpr uint32_t dlog_tag(uint64_t w0) { return (uint32_t)dlog_mix(w0); }
constexpr uint64_t dlog_slot_value(uint64_t w0, uint32_t j) { return ((uint64_t)dlog_tag(w0) << 32) | j; }
constexpr uint32_t dlog_slot_tag(uint64_t slot) { return (uint32_t)(slot >> 32); }
constexpr uint32_t dlog_slot_index(uint64_t slot) { return (uint32_t)slot; }
constexpr size_t dlog_next(size_t s, unsigned t) { return (s + 1) & (dlog_slots(t) - 1); }          // linear probing

// ---- insertion, on the host and in j order: the layout is a function of the records alone.
inline bool dlog_records_equal(const uint64_t* a, const uint64_t* b) { return a[0] == b[0] && a[1] == b[1] && a[2] == b[2] && a[3] == b[3]; }
// Files record j.  false: the very record is in the table already (two multiples of the generator coincide: the backstop of the
// E[8] refusal); the slots stay as they were.
inline bool dlog_insert(uint64_t* slots, unsigned t, const uint64_t* records, uint32_t j)
{
    const uint64_t w0 = records[4 * (size_t)j];
    const uint32_t tag = dlog_tag(w0);
    size_t s = dlog_home(w0, t);
    while (slots[s] != DLOG_EMPTY) {
        if (dlog_slot_tag(slots[s]) == tag && dlog_records_equal(records + 4 * (size_t)dlog_slot_index(slots[s]), records + 4 * (size_t)j)) return false;
        s = dlog_next(s, t);
    }
    slots[s] = dlog_slot_value(w0, j);
    return true;
}
// All 2^t records into 2^(t+1) slots.  Returns the first j that could not be filed, or -1.
inline long dlog_build_slots(uint64_t* slots, unsigned t, const uint64_t* records)
{
    for (size_t s = 0; s < dlog_slots(t); s++) slots[s] = DLOG_EMPTY;
    for (size_t j = 0; j < dlog_records(t); j++)
        if (!dlog_insert(slots, t, records, (uint32_t)j)) return (long)j;
    return -1;
}
// The lookup the kernels make, for the tests: the j whose record equals `rec` in words 0..3, or -1.
inline long dlog_find(const uint64_t* slots, unsigned t, const uint64_t* records, const uint64_t* rec)
{
    const uint32_t tag = dlog_tag(rec[0]);
    for (size_t s = dlog_home(rec[0], t); slots[s] != DLOG_EMPTY; s = dlog_next(s, t))
        if (dlog_slot_tag(slots[s]) == tag && dlog_records_equal(records + 4 * (size_t)dlog_slot_index(slots[s]), rec)) return (long)dlog_slot_index(slots[s]);
    return -1;
}

// ---- the setup block of a table (32-bit words), written by one lane at create time: word 0 the verdict, then records of
// DLOG_SETUP_STRIDE words from word DLOG_SETUP_STRIDE on.  A cached affine point is (Y - X, Y + X, 2 d X Y) of 9 words each.
constexpr int DLOG_SETUP_STRIDE = 32;
constexpr int DLOG_SETUP_G = 1;            // G_eff as a cached affine point
constexpr int DLOG_SETUP_S = 2;            // the stride S = -2^t * G_eff
constexpr int DLOG_SETUP_W = 3;            // W_0 .. W_63, W_k = k * DLOG_STEPS_PER_LAUNCH * S
constexpr size_t DLOG_SETUP_WORDS = (size_t)DLOG_SETUP_STRIDE * (DLOG_SETUP_W + DLOG_MAX_LAUNCHES);
constexpr uint32_t DLOG_SETUP_OK = 0, DLOG_SETUP_NOT_A_POINT = 1, DLOG_SETUP_SMALL_ORDER = 2;
// where launch k finds its offset W_k
constexpr size_t dlog_offset_word(uint64_t k) { return (size_t)DLOG_SETUP_STRIDE * (DLOG_SETUP_W + (size_t)k); }

// ---- bounds and launch slices.  m = g * 2^t + j: giant step g, baby step j.
constexpr uint64_t dlog_max_bound(unsigned t) { return DLOG_MAX_STEPS << t; }
constexpr bool dlog_bits_ok(unsigned t) { return t >= DLOG_MIN_BITS && t <= DLOG_MAX_BITS; }
constexpr bool dlog_bound_ok(uint64_t bound, unsigned t) { return bound >= 1 && bound <= dlog_max_bound(t); }
constexpr uint64_t dlog_steps(uint64_t bound, unsigned t) { return ((bound - 1) >> t) + 1; }       // giant steps that hold an m < bound
constexpr uint64_t dlog_launches(uint64_t bound, unsigned t) { return (dlog_steps(bound, t) + DLOG_STEPS_PER_LAUNCH - 1) / DLOG_STEPS_PER_LAUNCH; }
struct DlogSlice {
    uint64_t first = 0;      // first giant step of launch k: k * DLOG_STEPS_PER_LAUNCH, the multiple of the stride in W_k
    uint64_t steps = 0;      // giant steps the launch covers, 1 .. DLOG_STEPS_PER_LAUNCH
    uint64_t chunks = 0;     // chunks of DLOG_CHUNK steps it walks (the last may reach past `steps`: m < bound decides)
};
constexpr DlogSlice dlog_slice(uint64_t bound, unsigned t, uint64_t k)
{
    DlogSlice s;
    s.first = k * DLOG_STEPS_PER_LAUNCH;
    const uint64_t left = dlog_steps(bound, t) - s.first;
    s.steps = left < DLOG_STEPS_PER_LAUNCH ? left : DLOG_STEPS_PER_LAUNCH;
    s.chunks = (s.steps + DLOG_CHUNK - 1) / DLOG_CHUNK;
    return s;
}
static_assert(dlog_launches(dlog_max_bound(DLOG_MAX_BITS), DLOG_MAX_BITS) == DLOG_MAX_LAUNCHES, "every launch has its offset");

}  // namespace zc
