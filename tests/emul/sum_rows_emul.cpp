// sum_rows_emul.cpp -- TEST-ONLY host build of the device functions behind the point sums (zc_sum.hip.h: sum_slice_fold,
// sum_wire_slice_fold, sum_tree_pair, sum_tree_more, the partial records; zc_sum_plan.h: the plan).  The loops stand for the
// launches: per row the lanes of the first kernel one after another (a slice fold each), then the tree level by level over an
// array of partials laid out as the workspace is -- for every number of parts the same walk, since where a level runs (inside a
// workgroup or in the second kernel) changes no value.  Rows are independent by construction here; that they stay so on the
// device is the GPU tier's to show.  Never shipped.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../dusk_zerocaf_amd/csrc/zc_sum.hip.h"

extern "C" void zc_bound_fail(const char* what, int line)
{
    std::fprintf(stderr, "zc_arith.hip.h:%d: bound violated: %s\n", line, what);
    std::abort();
}

using namespace zc;

// The tree over the `parts` partials of one row in q (workspace layout), as the kernels run it; leaves the sum in element 0.
static void emul_tree(std::vector<u32>& q, size_t parts)
{
    std::vector<u32> next(q.size());
    for (size_t w = parts; sum_tree_more(w); w >>= 1) {
        for (size_t s = 0; s < (w >> 1); s++) {
            bool ok;
            const ptm r = sum_tree_pair(q.data(), s, SUM_PARTIAL_WORDS, 1, ok);
            sum_partial_put(next.data(), s, SUM_PARTIAL_WORDS, 1, r, ok);
        }
        std::memcpy(q.data(), next.data(), (w >> 1) * SUM_PARTIAL_WORDS * sizeof(u32));
    }
}

extern "C" {
size_t emul_sum_parts(size_t terms) { return sum_parts(terms); }
// what test_sum_rows_plan_emul.py reads of a plan: parts, steps, form, rows_per_block, blocks_per_row, grid1, grid2, partials,
// workspace_bytes
void emul_sum_plan(size_t n, size_t terms, uint64_t* out)
{
    const SumPlan p = sum_plan(n, terms);
    const uint64_t v[9] = {p.parts, p.steps, (uint64_t)p.form, p.rows_per_block, p.blocks_per_row, p.grid1, p.grid2, p.partials, p.workspace_bytes};
    std::memcpy(out, v, sizeof v);
}
uint32_t emul_sum_fold_steps(uint32_t terms, uint32_t parts) { return sum_fold_steps(terms, parts); }
// sum_ris_decode (the fold's decoder) against ris_decompress (zc_curve.hip.h) on n encodings: the number of encodings on which
// the verdicts or any canonical limb of the points differ
size_t emul_decode_differs(const uint8_t* in, size_t n)
{
    size_t bad = 0;
    for (size_t i = 0; i < n; i++) {
        u64 w[4], a[20], b[20];
        std::memcpy(w, in + 32 * i, 32);
        pt P, Q;
        const bool da = sum_ris_decode(P, w), db = ris_decompress(Q, w);
        pt_store(a, P);
        pt_store(b, Q);
        if (da != db || std::memcmp(a, b, sizeof a) != 0) bad++;
    }
    return bad;
}
int emul_sum_too_large(size_t n, size_t terms) { return sum_too_large(n, terms) ? 1 : 0; }
void emul_sum_constants(uint64_t* out)
{
    const uint64_t v[6] = {SUM_SERIAL_MAX, SUM_MIN_SLICE, SUM_MAX_PARTS, (uint64_t)SUM_BLOCK, SUM_PARTIAL_WORDS, SUM_INDEX_LIMIT};
    std::memcpy(out, v, sizeof v);
}
// k_ed_rowsum (+ k_ed_rowsum_finish): points n * terms * 20, out n * 20
void emul_ed_sum_rows(const u64* points, size_t terms, u64* out, size_t n)
{
    const SumPlan p = sum_plan(n, terms);
    std::vector<u32> q(p.parts * SUM_PARTIAL_WORDS);
    for (size_t i = 0; i < n; i++) {
        const u64* row = points + 20 * terms * i;
        for (size_t s = 0; s < p.parts; s++) {
            const ptm a = sum_slice_fold(terms, p.parts, s, sum_fold_steps((u32)terms, (u32)p.parts), [&](size_t, size_t j, bool have) { return have ? pt_load(row + 20 * j) : pt_identity(); });
            sum_partial_put(q.data(), s, SUM_PARTIAL_WORDS, 1, a, true);
        }
        emul_tree(q, p.parts);
        bool ok;
        sum_row_store(out + 20 * i, sum_partial_get(q.data(), 0, SUM_PARTIAL_WORDS, 1, ok));
    }
}
// k_ris_rowsum (+ k_ris_rowsum_finish): in n * terms * 32 bytes, out n * 32 bytes, okv n bytes or null
void emul_ris_sum_rows(const uint8_t* in, size_t terms, uint8_t* out, uint8_t* okv, size_t n)
{
    const SumPlan p = sum_plan(n, terms);
    std::vector<u32> q(p.parts * SUM_PARTIAL_WORDS);
    for (size_t i = 0; i < n; i++) {
        const uint8_t* row = in + 32 * terms * i;
        for (size_t s = 0; s < p.parts; s++) {
            bool ok;
            const ptm a = sum_wire_slice_fold(terms, p.parts, s, sum_fold_steps((u32)terms, (u32)p.parts), ok, [&](u64 (&w)[4], size_t j) { std::memcpy(w, row + 32 * j, 32); });
            sum_partial_put(q.data(), s, SUM_PARTIAL_WORDS, 1, a, ok);
        }
        emul_tree(q, p.parts);
        bool ok;
        const ptm a = sum_partial_get(q.data(), 0, SUM_PARTIAL_WORDS, 1, ok);
        u64 w[4];
        sum_row_encode(w, a, ok);
        std::memcpy(out + 32 * i, w, 32);
        if (okv) okv[i] = ok ? 1 : 0;
    }
}
}
