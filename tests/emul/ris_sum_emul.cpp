// ris_sum_emul.cpp -- TEST-ONLY host build of the device functions behind zc_ris_lincomb_sum (zc_ris_batch.hip.h:
// ris_sum_pair, ris_sum_row, sc_sum_strided / sc_sum_tree_step / sc_sum_store, ris_sum_store_basepoint).  The loops stand
// for the launches of k_ris_sum_prepare, k_ris_sum_rows and k_sc_sum: one call per lane, and for the reduction a workgroup
// is `block` lanes (a power of two) whose partials meet in an array where the kernel uses LDS, level by level as between
// the kernel's barriers.  Never shipped.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../dusk_zerocaf_amd/csrc/zc_ris_batch.hip.h"

extern "C" void zc_bound_fail(const char* what, int line)
{
    std::fprintf(stderr, "zc_arith.hip.h:%d: bound violated: %s\n", line, what);
    std::abort();
}

using namespace zc;

extern "C" {
// k_ris_sum_prepare: one lane per (row, term); z null = no weights.  in32 8-byte aligned as the kernel requires.
void emul_ris_sum_prepare(const uint8_t* in32, const u64* k, const u64* z, u64* points, u64* scalars, uint8_t* flags, size_t terms, size_t pairs)
{
    for (size_t g = 0; g < pairs; g++) {
        u64 w[4];
        std::memcpy(w, in32 + 32 * g, 32);
        ris_sum_pair(w, k + 5 * g, z ? z + 5 * (g / terms) : nullptr, points + 20 * g, scalars + 5 * g, flags + g);
    }
}
// k_ris_sum_rows: one lane per row
void emul_ris_sum_rows(const uint8_t* flags, u64* scalars, const u64* kb, const u64* z, uint8_t* ok, u64* t, u64* base_record, size_t terms, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        if (i == 0 && base_record) ris_sum_store_basepoint(base_record);
        ris_sum_row(flags + terms * i, terms, scalars + 5 * terms * i, kb ? kb + 5 * i : nullptr, z ? z + 5 * i : nullptr, ok ? ok + i : nullptr,
                    t ? t + 5 * i : nullptr);
    }
}
// one launch of k_sc_sum with `blocks` workgroups of `block` lanes: out[b] = workgroup b's sum
void emul_sc_sum_launch(const u64* t, size_t n, u64* out, size_t blocks, int block)
{
    std::vector<fe> part((size_t)block);
    for (size_t b = 0; b < blocks; b++) {
        for (int lane = 0; lane < block; lane++) part[(size_t)lane] = sc_sum_strided(t, n, b * (size_t)block + (size_t)lane, blocks * (size_t)block);
        for (int half = block / 2; half > 0; half >>= 1)
            for (int lane = 0; lane < half; lane++) sc_sum_tree_step(part.data(), lane, half);
        sc_sum_store(out + 5 * b, part[0]);
    }
}
// the host's two launches: `rows_per_lane` rows per lane of the first until `max_blocks` workgroups, one workgroup directly
void emul_sc_sum(const u64* t, size_t n, u64* out, int block, size_t rows_per_lane, size_t max_blocks)
{
    const size_t span = (size_t)block * rows_per_lane;
    size_t blocks = (n + span - 1) / span;
    if (blocks > max_blocks) blocks = max_blocks;
    if (blocks <= 1) {
        emul_sc_sum_launch(t, n, out, 1, block);
        return;
    }
    std::vector<u64> partial(5 * blocks);
    emul_sc_sum_launch(t, n, partial.data(), blocks, block);
    emul_sc_sum_launch(partial.data(), blocks, out, 1, block);
}
}
