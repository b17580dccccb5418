// lincomb_emul.cpp -- TEST-ONLY host build of the short-linear-combination core (k_ed_lincomb) on waves of 64 real lanes.
// The per-lane functions are the very ones the kernel calls (zc_curve.hip.h: load_scalar, scalar_recode16, lincomb_fast
// through table_ptr, lincomb_row_on_curve, lincomb_strict); the wave-level maximum of `top` is a loop over the lanes, so every lane of a wave runs the window
// loop from the same top window, as on the device.  Never shipped.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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
}

// Waves of 64 consecutive rows, the last one ragged (lanes past n run on row 0's data with top = -1, as in the kernel).
// points: n x terms x 20, scalars: n x terms x 5, out: n x 20.  tops: the wave-uniform top window of every wave.
// strict_rows: incremented for every row that failed the curve test and was evaluated by the reference's sequence.
extern "C" int emul_ed_lincomb(const u64* p, const u64* k, size_t terms, u64* out, size_t n, int* tops, int* strict_rows)
{
    if (terms < 1 || terms > (size_t)LINCOMB_MAX_TERMS) return -1;
    std::vector<u32> rw((size_t)WAVE * 9 * terms);                       // word w of term j of lane l at rw[(9 j + w) * WAVE + l]
    std::vector<u32> tables((size_t)WAVE * 256 * terms + 32);
    u32* aligned = tables.data();
    while (reinterpret_cast<uintptr_t>(aligned) & 127) aligned++;          // niels_load reads 128-byte records
    const size_t nwaves = (n + WAVE - 1) / WAVE;
    for (size_t w = 0; w < nwaves; w++) {
        int top = -1;
        for (int lane = 0; lane < WAVE; lane++) {
            const size_t i = w * WAVE + (size_t)lane;
            const bool valid = i < n;
            const size_t first = (valid ? i : 0) * terms;
            int lane_top = -1;
            for (size_t j = 0; j < terms; j++) {
                u64 l[5];
                load_scalar(l, k + 5 * (first + j));
                const int tj = scalar_recode16(rw.data() + 9 * j * WAVE + lane, WAVE, l);
                lane_top = tj > lane_top ? tj : lane_top;
            }
            if (!valid) lane_top = -1;
            top = lane_top > top ? lane_top : top;                         // wave_max_small
        }
        if (tops) tops[w] = top;
        for (int lane = 0; lane < WAVE; lane++) {
            const size_t i = w * WAVE + (size_t)lane;
            const size_t first = (i < n ? i : 0) * terms;
            pt Q = lincomb_fast(p + 20 * first, table_ptr{aligned + (size_t)lane * 256 * terms}, rw.data() + lane, WAVE, (int)terms, top);
            if (i < n && !lincomb_row_on_curve(p + 20 * first, (int)terms)) {          // k_ed_lincomb_off_curve_rows
                Q = lincomb_strict(p + 20 * first, k + 5 * first, (int)terms, rw.data() + lane, WAVE);
                if (strict_rows) ++*strict_rows;
            }
            if (i < n) pt_store(out + 20 * i, Q);
        }
    }
    return 0;
}

// the digits the window loop reads (scalar_recode16 / recoded_digit) next to the stored ones (scalar_digits16)
extern "C" void emul_lincomb_digits(const u64* k, int8_t* recoded, int8_t* stored, int* tops, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        u64 l[5];
        load_scalar(l, k + 5 * i);
        u32 rw[9];
        tops[2 * i] = scalar_recode16(rw, 1, l);
        tops[2 * i + 1] = scalar_digits16(stored + 66 * i, 1, l);
        for (int d = 0; d < 66; d++) recoded[66 * i + d] = (int8_t)recoded_digit(rw, 1, d);
    }
}

// the single-term windowed multiplication (scalar_mul_fast), for the terms == 1 comparison
extern "C" void emul_ed_scalar_mul_fast(const u64* p, const u64* k, u64* out, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        u64 l[5];
        load_scalar(l, k + 5 * i);
        alignas(128) u32 table[256];
        int8_t dig[66];
        const int top = scalar_digits16(dig, 1, l);
        pt_store(out + 20 * i, scalar_mul_fast(pt_load(p + 20 * i), table_ptr{table}, dig, 1, top));
    }
}
