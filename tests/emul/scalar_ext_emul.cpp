// scalar_ext_emul.cpp -- TEST-ONLY host build of the device functions behind zc_sc_from_bytes_wide / _mod_order, zc_sc_muladd
// and zc_sc_invert (zc_arith.hip.h: sc_reduce_words, sc_muladd_limbs52; zc_curve.hip.h: sc_invert_limbs52,
// mod_invert_chunk<ModL>).  The loops stand for the launches of k_sc_* in zc_kernels.hip.h: one call per lane, and for the
// shared inversions lane g of `lanes` takes the rows g, g + lanes, ... as k_sc_invert_chunked does.  Never shipped.
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
void words_at(u64 (&w)[4], const uint8_t* p)              // as load_words256_any: no alignment promise
{
    for (int i = 0; i < 4; i++) std::memcpy(&w[i], p + 8 * i, 8);
}
}  // namespace

extern "C" {
void emul_sc_from_bytes_wide(const uint8_t* in, u64* out, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        u64 lo[4], hi[4], l[5];
        words_at(lo, in + 64 * i);
        words_at(hi, in + 64 * i + 32);
        fe_to_limbs52(l, sc_reduce_words<true>(lo, hi));
        store5(out + 5 * i, l);
    }
}
void emul_sc_from_bytes_mod_order(const uint8_t* in, u64* out, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        u64 lo[4], hi[4] = {0, 0, 0, 0}, l[5];
        words_at(lo, in + 32 * i);
        fe_to_limbs52(l, sc_reduce_words<false>(lo, hi));
        store5(out + 5 * i, l);
    }
}
void emul_sc_muladd(const u64* a, const u64* b, const u64* c, u64* out, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        u64 x[5], y[5], z[5], r[5];
        load5(x, a + 5 * i);
        load5(y, b + 5 * i);
        load5(z, c + 5 * i);
        sc_muladd_limbs52(r, x, y, z);
        store5(out + 5 * i, r);
    }
}
// zc_sc_mul's own function (fe_mulmod_limbs52<ModL>): the multiplier a a^-1 = 1 is checked with
void emul_sc_mul(const u64* a, const u64* b, u64* out, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        u64 x[5], y[5], r[5];
        load5(x, a + 5 * i);
        load5(y, b + 5 * i);
        fe_mulmod_limbs52<ModL>(r, x, y);
        store5(out + 5 * i, r);
    }
}
void emul_sc_invert(const u64* a, u64* out, uint8_t* ok, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        u64 l[5], r[5];
        load5(l, a + 5 * i);
        bool nz;
        sc_invert_limbs52(r, &nz, l);
        store5(out + 5 * i, r);
        if (ok) ok[i] = nz ? 1 : 0;
    }
}
// ilp != 0: k_sc_invert_chunked_lone (the independent-chain multiplier)
void emul_sc_invert_chunked(const u64* a, u64* out, uint8_t* ok, size_t n, int c, int ilp)
{
    const size_t lanes = (n + (size_t)c - 1) / (size_t)c;
    for (size_t g = 0; g < lanes; g++) {
        if (ilp) mod_invert_chunk<ModL, true>(a, out, ok, n, g, lanes, c);
        else mod_invert_chunk<ModL, false>(a, out, ok, n, g, lanes, c);
    }
}
}
