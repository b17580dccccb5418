// shared_lincomb_emul.cpp -- TEST-ONLY host build of the device functions behind zc_ed_lincomb_shared and zc_ris_lincomb_shared
// (zc_shared.hip.h: the partial tables of odd multiples, the loop over the host's joint schedule, the wire form's decode-into-
// table steps and the fused double-and-encode), with the host's own merge of the scalar vector (zc_shared_scalar.h) in front, as
// zerocaf_hip.hip calls it.  The loops stand for the launches: one call per lane, the lane's 1 KB of table per term in a local
// array (table_ptr: term j at 256 * j words).  Never shipped.
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
pt lane_sum(const table_ptr t, const shared_lincomb_schedule& s, int ilp)
{
    const pt Q = ilp ? shared_lincomb_steps<true>(t, s) : shared_lincomb_steps<false>(t, s);
    return ilp ? shared_doublings<true>(Q, s.tail) : shared_doublings<false>(Q, s.tail);
}
}  // namespace

extern "C" {
// k_ed_lincomb_shared: points n * terms * 20, k terms * 5; out may be points for terms == 1
void emul_ed_lincomb_shared(const u64* points, const u64* k, size_t terms, u64* out, size_t n, int ilp)
{
    const shared_lincomb_schedule s = shared_lincomb_schedule_ed(k, terms);
    for (size_t i = 0; i < n; i++) {
        alignas(128) u32 table[256 * SHARED_LINCOMB_MAX_TERMS];
        std::memset(table, 0xA5, sizeof table);             // a record the schedule never names holds no point
        const table_ptr t{table};
        for (u32 j = 0; j < s.terms; j++)
            if (s.entries[j]) shared_table_build_upto(pt_load(points + 20 * (i * terms + j)), t.term((int)j), s.entries[j]);
        pt_store(out + 20 * i, lane_sum(t, s, ilp));
    }
}
// k_ris_lincomb_shared: in32 n * terms * 32; ok may be null
void emul_ris_lincomb_shared(const uint8_t* in32, const u64* k, size_t terms, uint8_t* out32, uint8_t* ok, size_t n, int ilp)
{
    const shared_lincomb_schedule s = shared_lincomb_schedule_wire(k, terms);
    for (size_t i = 0; i < n; i++) {
        alignas(128) u32 table[256 * SHARED_LINCOMB_MAX_TERMS];
        std::memset(table, 0xA5, sizeof table);
        const table_ptr t{table};
        bool dec = true;
        for (u32 j = 0; j < s.terms; j++) {
            u64 w[4];
            std::memcpy(w, in32 + 32 * (i * terms + j), 32);
            dec = shared_lincomb_decode(w, t.term((int)j)) && dec;
        }
        for (u32 j = 0; j < s.terms; j++) shared_lincomb_table(t.term((int)j), s.entries[j]);
        u64 w[4];
        shared_ris_encode(w, lane_sum(t, s, ilp), dec);
        std::memcpy(out32 + 32 * i, w, 32);
        if (ok) ok[i] = dec ? 1 : 0;
    }
}
}
