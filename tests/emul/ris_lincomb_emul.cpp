// ris_lincomb_emul.cpp -- TEST-ONLY host build of the wire-format linear-combination core (k_ris_lincomb) on waves of 64 real
// lanes.  The per-lane functions are the very ones the kernel calls (zc_curve.hip.h: ris_lincomb_decode, ris_lincomb_table,
// scalar_recode16, scalar_recode256, ris_lincomb_sum, base_mul_onto, ris_lincomb_encode, through table_ptr); the comb table
// is built by the kernel's column arithmetic (base_table_column); the wave-level maxima of the two top digits are loops over
// the lanes, so every lane of a wave runs both loops from the same top, as on the device.  Never shipped.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../dusk_zerocaf_amd/csrc/zc_curve.hip.h"

extern "C" void zc_bound_fail(const char* what, int line)
{
    std::fprintf(stderr, "zc_arith.hip.h:%d: bound violated: %s\n", line, what);
    std::abort();
}

using namespace zc;

namespace {
constexpr int WAVE = 64;
u32* aligned128(std::vector<u32>& v)
{
    u32* p = v.data();
    while (reinterpret_cast<uintptr_t>(p) & 127) p++;                          // niels_load reads 128-byte records
    return p;
}
// the basepoint comb, 33 x 128 records of 32 words, built once by the columns k_base_table_build's lanes build
const u32* comb_table()
{
    static std::vector<u32> store;
    static u32* table = nullptr;
    if (!table) {
        store.resize((size_t)ZC_BASE_WINDOWS * ZC_BASE_ENTRIES * 32 + 32);
        table = aligned128(store);
        for (int j = 0; j < ZC_BASE_ENTRIES; j++) base_table_column(table, j);
    }
    return table;
}
}

// Waves of 64 consecutive rows, the last one ragged (lanes past n run on row 0's data with top = -1, as in the kernel).
// in: n x terms x 32 bytes, k: n x terms x 5, kb: null or n x 5, out: n x 32 bytes, ok: n bytes.
// tops: two entries per wave, the wave-uniform top window of the terms and the top digit of the base scalars.
extern "C" int emul_ris_lincomb(const uint8_t* in, const u64* k, size_t terms, const u64* kb, uint8_t* out, uint8_t* ok, size_t n, int* tops)
{
    const size_t slots = terms + (kb ? 1 : 0);
    if (terms < 1 || slots > (size_t)LINCOMB_MAX_TERMS) return -1;
    std::vector<u32> rw((size_t)WAVE * 9 * slots);                             // word w of slot j of lane l at rw[(9 j + w) * WAVE + l]
    std::vector<u32> tables((size_t)WAVE * 256 * terms + 32);
    u32* const aligned = aligned128(tables);
    const u32* const comb = kb ? comb_table() : nullptr;
    const size_t nwaves = (n + WAVE - 1) / WAVE;
    for (size_t w = 0; w < nwaves; w++) {
        bool dec[WAVE];
        int top = -1, base_top = -1;
        for (int lane = 0; lane < WAVE; lane++) {
            const size_t i = w * WAVE + (size_t)lane;
            const bool valid = i < n;
            const size_t row = valid ? i : 0, first = row * terms;
            const table_ptr mine{aligned + (size_t)lane * 256 * terms};
            dec[lane] = true;
            for (size_t j = 0; j < terms; j++) {
                u64 words[4];
                std::memcpy(words, in + 32 * (first + j), 32);
                dec[lane] = ris_lincomb_decode(words, mine.term((int)j)) && dec[lane];
            }
            for (size_t j = 0; j < terms; j++) ris_lincomb_table(mine.term((int)j));
            int lane_top = -1, lane_base_top = -1;
            for (size_t j = 0; j < terms; j++) {
                u64 l[5];
                load_scalar(l, k + 5 * (first + j));
                const int tj = scalar_recode16(rw.data() + 9 * j * WAVE + lane, WAVE, l);
                lane_top = tj > lane_top ? tj : lane_top;
            }
            if (kb) {
                u64 l[5];
                load_scalar(l, kb + 5 * row);
                lane_base_top = scalar_recode256(rw.data() + 9 * terms * WAVE + lane, WAVE, l);
            }
            if (!valid || !dec[lane]) lane_top = lane_base_top = -1;
            top = lane_top > top ? lane_top : top;                             // wave_max_small
            base_top = lane_base_top > base_top ? lane_base_top : base_top;
        }
        if (tops) {
            tops[2 * w] = top;
            tops[2 * w + 1] = base_top;
        }
        for (int lane = 0; lane < WAVE; lane++) {
            const size_t i = w * WAVE + (size_t)lane;
            pt Q = ris_lincomb_sum(table_ptr{aligned + (size_t)lane * 256 * terms}, rw.data() + lane, WAVE, (int)terms, top);
            if (kb) Q = base_mul_onto(Q, comb, rw.data() + 9 * terms * WAVE + lane, WAVE, base_top);
            u64 words[4];
            ris_lincomb_encode(words, Q, dec[lane]);
            if (i < n) {
                std::memcpy(out + 32 * i, words, 32);
                ok[i] = dec[lane] ? 1 : 0;
            }
        }
    }
    return 0;
}

// the base digits the comb additions read (scalar_recode256 / recoded_digit256) next to the stored ones (scalar_digits256)
extern "C" void emul_base_digits(const u64* k, int8_t* recoded, int8_t* stored, int* tops, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        u64 l[5];
        load_scalar(l, k + 5 * i);
        u32 rw[9];
        tops[2 * i] = scalar_recode256(rw, 1, l);
        tops[2 * i + 1] = scalar_digits256(stored + ZC_BASE_WINDOWS * i, 1, l);
        for (int d = 0; d < ZC_BASE_WINDOWS; d++) recoded[ZC_BASE_WINDOWS * i + d] = (int8_t)recoded_digit256(rw, 1, d);
    }
}

// k * B from the host-built comb with the kernels' own base_mul (k_ed_mul_base): checks the table the rows above add from
extern "C" void emul_ed_mul_base(const u64* k, u64* out, size_t n)
{
    const u32* const comb = comb_table();
    for (size_t i = 0; i < n; i++) {
        u64 l[5];
        load_scalar(l, k + 5 * i);
        int8_t dig[ZC_BASE_WINDOWS];
        const int top = scalar_digits256(dig, 1, l);
        pt_store(out + 20 * i, base_mul(comb, dig, 1, top));
    }
}
