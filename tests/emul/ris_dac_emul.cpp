// ris_dac_emul.cpp -- TEST-ONLY host build of the device functions behind zc_ris_double_and_compress
// (zc_ris_batch.hip.h: ris_double_compress_row, ris_double_compress_chunk).  The loops stand for the launches of
// k_ris_double_compress*: one call per lane, and for the shared inversions lane g of `lanes` takes the rows g, g + lanes, ...
// as k_ris_double_compress_chunked does.  Never shipped.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../dusk_zerocaf_amd/csrc/zc_ris_batch.hip.h"

extern "C" void zc_bound_fail(const char* what, int line)
{
    std::fprintf(stderr, "zc_arith.hip.h:%d: bound violated: %s\n", line, what);
    std::abort();
}

using namespace zc;

extern "C" {
// k_ris_double_compress: one row per lane
void emul_ris_dac_rows(const u64* p, uint8_t* out32, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        u64 w[4];
        ris_double_compress_row(w, p + 20 * i);
        std::memcpy(out32 + 32 * i, w, 32);
    }
}
// k_ris_double_compress_chunked (ilp != 0: _lone, the independent-chain multiplier); out32 8-byte aligned as the kernel requires
void emul_ris_dac_chunked(const u64* p, uint8_t* out32, size_t n, int c, int ilp)
{
    const size_t lanes = (n + (size_t)c - 1) / (size_t)c;
    for (size_t g = 0; g < lanes; g++) {
        if (ilp) ris_double_compress_chunk<true>(p, out32, n, g, lanes, c);
        else ris_double_compress_chunk<false>(p, out32, n, g, lanes, c);
    }
}
}
