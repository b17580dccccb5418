// zc_shared_scalar.h -- what the host does with the ONE scalar of zc_ed_scalar_mul_shared / zc_ris_mul_shared before it
// launches (zerocaf_hip.hip), and the schedule the kernels of zc_shared.hip.h walk.  Plain C++17 without any HIP include:
// tests/test_shared_scalar_plan_emul.py drives it on the CPU.
//
//   shared_effective   the value double_and_add multiplies by (the rule of zc_curve.hip.h: scalar_effective): limb bits from
//                      2^52 up are masked, and a pattern v >= 2^256 whose low 256 bits lie below 2^ctz(v >> 256) loses its high bits
//   shared_half_mod_l  k' = (k_eff mod L) * 2^-1 mod L on 64-bit words: the wire form multiplies by k' and leaves through the
//                      double-and-encode formula (zc_ris_batch.hip.h), since encode(k P) = encode(2 (k' P)) for a decoded P
//   shared_recode      the width-5 signed sliding window of a value below 2^260: v = sum d_i 2^(p_i), every d_i odd and
//                      |d_i| <= 15, p_(i+1) >= p_i + 5 -- so at most ceil(261 / 5) = 53 digits -- as a list of steps from
//                      the top digit down: {doublings before the addition, digit}, then the doublings after the last one
//
// The schedule is a fixed-size POD and travels BY VALUE in the kernel arguments (220 bytes): every wave reads it through
// the scalar cache, no lane keeps a digit, and nothing of the scalar stays in device memory after the launch.
#pragma once
#include <cstddef>
#include <cstdint>

namespace zc {

constexpr int SHARED_WINDOW = 5;
constexpr int SHARED_MAX_STEPS = 53;                   // ceil(261 / 5): a 260-bit value has at most 261 signed digits

// step word: bits 0..15 the doublings before the addition (0 for the first step, which starts from the identity, then
// 5 .. 260), bits 16..23 the digit as a two's complement byte (odd, -15 .. 15)
struct shared_schedule {
    uint32_t steps;                                    // additions, 0 .. 53 (0: the scalar is zero)
    uint32_t tail;                                     // doublings after the last addition (the position of the lowest digit)
    uint32_t step[SHARED_MAX_STEPS];
};
constexpr uint32_t shared_step_word(unsigned doublings, int digit) { return (uint32_t)doublings | ((uint32_t)(uint8_t)(int8_t)digit << 16); }
constexpr uint32_t shared_step_doublings(uint32_t w) { return w & 0xFFFFu; }
constexpr int shared_step_digit(uint32_t w) { return (int)(int8_t)(uint8_t)(w >> 16); }

// a 320-bit little-endian integer
struct shared_words {
    uint64_t w[5];
};

// L = 2^249 + 14490550575682688738086195780655237219, the order of the prime subgroup
constexpr shared_words SHARED_L = {{0x6ab4036f755fc863ull, 0x0ae6c74d822fd593ull, 0x0ull, 0x0200000000000000ull, 0x0ull}};

// The limbs double_and_add's loop actually consumes (see scalar_effective in zc_curve.hip.h for the derivation).
inline void shared_effective(uint64_t (&l)[5], const uint64_t* k)
{
    const uint64_t m52 = ((uint64_t)1 << 52) - 1, low48 = ((uint64_t)1 << 48) - 1;
    for (int j = 0; j < 5; j++) l[j] = k[j] & m52;
    const uint32_t hi = (uint32_t)(l[4] >> 48);
    if (hi) {
        const int tz = __builtin_ctz(hi);
        const bool stops_early = (l[1] | l[2] | l[3] | (l[4] & low48)) == 0 && l[0] < ((uint64_t)1 << tz);
        if (stops_early) l[4] &= low48;
    }
}
// five 52-bit limbs -> the integer
inline shared_words shared_from_limbs52(const uint64_t (&l)[5])
{
    shared_words v = {{0, 0, 0, 0, 0}};
    for (int j = 0; j < 5; j++) {
        const int bit = 52 * j, word = bit / 64, sh = bit % 64;
        v.w[word] |= l[j] << sh;
        if (sh > 12) v.w[word + 1] |= l[j] >> (64 - sh);           // 52 + sh > 64; word + 1 <= 4 since 52 * 4 + 52 = 260 < 320
    }
    return v;
}
// the integer (below 2^260) -> five 52-bit limbs
inline void shared_to_limbs52(uint64_t (&l)[5], const shared_words& v)
{
    const uint64_t m52 = ((uint64_t)1 << 52) - 1;
    for (int j = 0; j < 5; j++) {
        const int bit = 52 * j, word = bit / 64, sh = bit % 64;
        uint64_t x = v.w[word] >> sh;
        if (sh > 12) x |= v.w[word + 1] << (64 - sh);
        l[j] = x & m52;
    }
}
inline shared_words shared_shl(const shared_words& a, int s)      // 0 <= s < 64, no bit leaves the 320
{
    shared_words r;
    for (int j = 4; j >= 0; j--) r.w[j] = (a.w[j] << s) | (s && j ? a.w[j - 1] >> (64 - s) : 0);
    return r;
}
inline bool shared_geq(const shared_words& a, const shared_words& b)
{
    for (int j = 4; j >= 0; j--)
        if (a.w[j] != b.w[j]) return a.w[j] > b.w[j];
    return true;
}
inline shared_words shared_sub(const shared_words& a, const shared_words& b)      // a >= b
{
    shared_words r;
    uint64_t borrow = 0;
    for (int j = 0; j < 5; j++) {
        const uint64_t x = a.w[j] - b.w[j], y = x - borrow;
        borrow = (a.w[j] < b.w[j]) | (x < borrow);
        r.w[j] = y;
    }
    return r;
}
inline shared_words shared_add(const shared_words& a, const shared_words& b)      // the sum stays below 2^320
{
    shared_words r;
    uint64_t carry = 0;
    for (int j = 0; j < 5; j++) {
        const uint64_t x = a.w[j] + b.w[j], y = x + carry;
        carry = (x < a.w[j]) | (y < x);
        r.w[j] = y;
    }
    return r;
}
// (v mod L) * 2^-1 mod L for v < 2^260 < 2^11 L: shifted subtractions of L, then v / 2 or (v + L) / 2
inline shared_words shared_half_mod_l(shared_words v)
{
    for (int s = 11; s >= 0; s--) {
        const shared_words ls = shared_shl(SHARED_L, s);
        if (shared_geq(v, ls)) v = shared_sub(v, ls);
    }
    if (v.w[0] & 1) v = shared_add(v, SHARED_L);
    for (int j = 0; j < 5; j++) v.w[j] = (v.w[j] >> 1) | (j < 4 ? v.w[j + 1] << 63 : 0);
    return v;
}
// the schedule of v < 2^260
inline shared_schedule shared_recode(shared_words v)
{
    int pos[SHARED_MAX_STEPS + 1], dig[SHARED_MAX_STEPS + 1], cnt = 0;
    for (int bit = 0; bit < 320 && cnt <= SHARED_MAX_STEPS; bit++) {
        if ((v.w[0] | v.w[1] | v.w[2] | v.w[3] | v.w[4]) == 0) break;
        if (v.w[0] & 1) {
            int d = (int)(v.w[0] & ((1u << SHARED_WINDOW) - 1));
            if (d >= (1 << (SHARED_WINDOW - 1))) d -= 1 << SHARED_WINDOW;
            const shared_words m = {{(uint64_t)(d < 0 ? -d : d), 0, 0, 0, 0}};
            v = d < 0 ? shared_add(v, m) : shared_sub(v, m);          // the low five bits are now zero
            pos[cnt] = bit;
            dig[cnt] = d;
            cnt++;
        }
        for (int j = 0; j < 5; j++) v.w[j] = (v.w[j] >> 1) | (j < 4 ? v.w[j + 1] << 63 : 0);
    }
    shared_schedule s = {};
    if (cnt > SHARED_MAX_STEPS) cnt = SHARED_MAX_STEPS;               // unreachable below 2^260 (the emulation tests the bound)
    s.steps = (uint32_t)cnt;
    s.tail = cnt ? (uint32_t)pos[0] : 0;
    for (int i = 0; i < cnt; i++) {
        const int at = cnt - 1 - i;                                   // from the top digit down
        s.step[i] = shared_step_word(i ? (unsigned)(pos[at + 1] - pos[at]) : 0u, dig[at]);
    }
    return s;
}

// What a call does with its scalar: the Edwards form walks k_eff itself, the wire form k' = (k_eff mod L) / 2 mod L.
inline shared_schedule shared_schedule_ed(const uint64_t* k)
{
    uint64_t l[5];
    shared_effective(l, k);
    return shared_recode(shared_from_limbs52(l));
}
inline shared_schedule shared_schedule_wire(const uint64_t* k)
{
    uint64_t l[5];
    shared_effective(l, k);
    return shared_recode(shared_half_mod_l(shared_from_limbs52(l)));
}

// ---------------------------------------------------------------- a scalar VECTOR for the batch (zc_ed_lincomb_shared / zc_ris_lincomb_shared)
// out[i] = sum_j k_j P_ij with the k_j shared by every row: each term is recoded as above and the digits of all terms are
// merged into ONE list from the top position down -- one doubling chain, one cached addition per non-zero digit of any term.
// A step word is shared_schedule's with the term index in its spare bits 24..31; two terms with a digit at the same position
// give a step with 0 doublings in front (ties in term order).  At most 53 * terms steps.  entries[j]: how many records of
// term j's table {1, 3, .., 15} P_ij the schedule reads, (max |d| + 1) / 2 -- 0 for a zero scalar, 1 for +-2^e -- so that
// the kernels build no more than that.  1 740 bytes, by value in the kernel arguments like shared_schedule.
constexpr int SHARED_LINCOMB_MAX_TERMS = 8;
constexpr int SHARED_LINCOMB_MAX_STEPS = SHARED_MAX_STEPS * SHARED_LINCOMB_MAX_TERMS;
struct shared_lincomb_schedule {
    uint32_t steps;                                    // additions, 0 .. 53 * terms
    uint32_t tail;                                     // doublings after the last addition
    uint32_t terms;                                    // 1 .. 8
    uint32_t entries[SHARED_LINCOMB_MAX_TERMS];        // table records term j needs, 0 .. 8
    uint32_t step[SHARED_LINCOMB_MAX_STEPS];
};
static_assert(sizeof(shared_lincomb_schedule) == 4 * (3 + SHARED_LINCOMB_MAX_TERMS + SHARED_LINCOMB_MAX_STEPS), "a POD of 32-bit words");
static_assert(sizeof(shared_lincomb_schedule) + 256 <= 2048, "the schedule and the other kernel arguments stay well under the 4 KB of kernel arguments");
constexpr uint32_t shared_lincomb_step_word(unsigned doublings, int digit, unsigned term) { return shared_step_word(doublings, digit) | ((uint32_t)term << 24); }
constexpr unsigned shared_step_term(uint32_t w) { return w >> 24; }

// The merge of the terms' schedules.  Term j's digit positions follow from its tail and its doublings; the next step is
// always the highest position any term still holds, the lowest term index first.
inline shared_lincomb_schedule shared_lincomb_merge(const shared_schedule* per_term, size_t terms)
{
    shared_lincomb_schedule s = {};
    if (terms > (size_t)SHARED_LINCOMB_MAX_TERMS) terms = SHARED_LINCOMB_MAX_TERMS;       // the entry points refuse such a call
    s.terms = (uint32_t)terms;
    int pos[SHARED_LINCOMB_MAX_TERMS][SHARED_MAX_STEPS];
    uint32_t at[SHARED_LINCOMB_MAX_TERMS];
    for (size_t j = 0; j < terms; j++) {
        const shared_schedule& t = per_term[j];
        int p = (int)t.tail, maxabs = 0;
        for (int i = (int)t.steps - 1; i >= 0; i--) {
            pos[j][i] = p;
            p += (int)shared_step_doublings(t.step[i]);
            const int d = shared_step_digit(t.step[i]), a = d < 0 ? -d : d;
            maxabs = a > maxabs ? a : maxabs;
        }
        s.entries[j] = (uint32_t)((maxabs + 1) / 2);
        at[j] = 0;
    }
    int last = 0;
    for (;;) {
        int best = -1;
        for (size_t j = 0; j < terms; j++)
            if (at[j] < per_term[j].steps && (best < 0 || pos[j][at[j]] > pos[best][at[best]])) best = (int)j;
        if (best < 0) break;
        const int p = pos[best][at[best]];
        s.step[s.steps] = shared_lincomb_step_word(s.steps ? (unsigned)(last - p) : 0u, shared_step_digit(per_term[best].step[at[best]]), (unsigned)best);
        s.steps++;
        at[best]++;
        last = p;
    }
    s.tail = (uint32_t)last;
    return s;
}
// k: terms * 5 words.  The Edwards form walks the k_eff,j themselves, the wire form the k'_j = (k_eff,j mod L) / 2 mod L.
inline shared_lincomb_schedule shared_lincomb_schedule_ed(const uint64_t* k, size_t terms)
{
    shared_schedule per_term[SHARED_LINCOMB_MAX_TERMS];
    for (size_t j = 0; j < terms && j < (size_t)SHARED_LINCOMB_MAX_TERMS; j++) per_term[j] = shared_schedule_ed(k + 5 * j);
    return shared_lincomb_merge(per_term, terms);
}
inline shared_lincomb_schedule shared_lincomb_schedule_wire(const uint64_t* k, size_t terms)
{
    shared_schedule per_term[SHARED_LINCOMB_MAX_TERMS];
    for (size_t j = 0; j < terms && j < (size_t)SHARED_LINCOMB_MAX_TERMS; j++) per_term[j] = shared_schedule_wire(k + 5 * j);
    return shared_lincomb_merge(per_term, terms);
}

}  // namespace zc
