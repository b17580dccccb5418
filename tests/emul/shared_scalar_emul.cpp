// shared_scalar_emul.cpp -- TEST-ONLY host build of the device functions behind zc_ed_scalar_mul_shared and zc_ris_mul_shared
// (zc_shared.hip.h: the table of odd multiples, the loop over the host's schedule, the fused double-and-encode), with the
// host's own recoding of the scalar (zc_shared_scalar.h) in front, as zerocaf_hip.hip calls it.  The loops stand for the
// launches: one call per lane, the lane's 1 KB of table in a local array (table_ptr).  Never shipped.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../dusk_zerocaf_amd/csrc/zc_shared.hip.h"

extern "C" void zc_bound_fail(const char* what, int line)
{
    std::fprintf(stderr, "zc_arith.hip.h:%d: bound violated: %s\n", line, what);
    std::abort();
}

using namespace zc;

namespace {
// one lane of either kernel between its loads and its stores (ilp: the form small launches take)
pt lane_mul(const pt& P, const shared_schedule& s, int ilp)
{
    alignas(128) u32 table[256];
    const table_ptr t{table};
    shared_table_build(P, t);
    return ilp ? shared_tail<true>(shared_steps<true>(t, s), s) : shared_tail<false>(shared_steps<false>(t, s), s);
}
}  // namespace

extern "C" {
// k_ed_scalar_mul_shared; out may be p
void emul_ed_scalar_mul_shared(const u64* p, const u64* k, u64* out, size_t n, int ilp)
{
    const shared_schedule s = shared_schedule_ed(k);
    for (size_t i = 0; i < n; i++) pt_store(out + 20 * i, lane_mul(pt_load(p + 20 * i), s, ilp));
}
// k_ris_mul_shared; out32 may be in32, ok may be null
void emul_ris_mul_shared(const uint8_t* in32, const u64* k, uint8_t* out32, uint8_t* ok, size_t n, int ilp)
{
    const shared_schedule s = shared_schedule_wire(k);
    for (size_t i = 0; i < n; i++) {
        u64 w[4];
        std::memcpy(w, in32 + 32 * i, 32);
        pt P;
        const bool dec = shared_ris_decode(P, w);
        shared_ris_encode(w, lane_mul(P, s, ilp), dec);
        std::memcpy(out32 + 32 * i, w, 32);
        if (ok) ok[i] = dec ? 1 : 0;
    }
}
}
