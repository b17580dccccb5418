// zc_scvec_plan.h -- what the scalar vector ops (zerocaf_hip.hip: zc_sc_sum_rows, zc_sc_dot_rows, zc_sc_powers; kernels in
// zc_scvec.hip.h) derive from (n, terms) before they touch the device: the cut of a row into slices, the kernel form, the grids,
// the workspace, the lane group of the powers and the index limit.  Plain C++17 without any HIP include:
// tests/test_scvec_plan_emul.py drives it on the CPU.  No knob reads into it.  Addition mod L is associative and every result is
// canonical, so nothing here changes a result: the plan only places the work.
#pragma once
#include <cstddef>
#include <cstdint>

namespace zc {

constexpr int SCV_BLOCK = 256;                       // lanes of a workgroup
constexpr size_t SCV_INDEX_LIMIT = (size_t)1 << 31;  // n * terms stays below this
constexpr size_t SCV_PARTIAL_WORDS = 10;             // 32-bit words of a partial in the workspace: nine canonical limbs, one unused

// ---- sums and dot products.  A row of `terms` records is cut into P = scv_parts(terms) slices, slice s holding the records
// s, s + P, s + 2 P, ... (consecutive lanes take consecutive records); a lane folds one slice, the P partials are added in a tree.
//   terms <= SCV_BLOCK_TERMS_MAX   BLOCK: P = 1, 4, 16, 64, 256 with terms <= 4 P, 256 / P rows per workgroup, at most four records
//                            per lane.  The workgroup's rows are ONE contiguous block of at most SCV_STAGE records, staged whole.
//   terms <= SCV_P256_MAX    ROW: P = 256, one row per workgroup, two steps of 256 consecutive records staged at a time
//   above                    TWO: P = 256 * bpr, bpr = min(SCV_MAX_BPR, ceil(terms / SCV_TWO_ROW_TERMS)) workgroups per row leave one
//                            partial each in the workspace; a second kernel adds a row's bpr partials (any count, odd ones too)
constexpr size_t SCV_STAGE = 1024;                   // records of 40 bytes a workgroup of the block form stages
constexpr size_t SCV_BLOCK_TERMS_MAX = 1024;
constexpr size_t SCV_P256_MAX = 32768;
constexpr size_t SCV_TWO_ROW_TERMS = 16384;          // records a workgroup of the two-kernel form takes when it can: 64 per lane
constexpr size_t SCV_MAX_BPR = 4096;                 // a lane of the second kernel adds at most 16 partials before the tree
constexpr size_t SCV_LONG_STAGE_STEPS = 2;           // steps the long forms stage at a time
// The dot product adds the 17 columns of every product into 64-bit accumulators and carries after SCV_CARRY_EVERY products: one
// column of one product of two 260-bit values stays below 9 * 2^58, seven of them and a carried-in limb below 2^64.
constexpr size_t SCV_CARRY_EVERY = 7;
// A slice of m products of 260-bit values is below m * 2^520: up to this many products it stays below 2^522, eighteen limbs of 29
// bits, and the fold has no nineteenth limb to bring in (zc_scvec.hip.h: scv_cols_fold).  The block form's slices are that short.
constexpr size_t SCV_NOHI_MAX = 4;

inline size_t scv_bpr(size_t terms)
{
    const size_t want = (terms + SCV_TWO_ROW_TERMS - 1) / SCV_TWO_ROW_TERMS;
    return want < SCV_MAX_BPR ? want : SCV_MAX_BPR;
}
inline size_t scv_parts(size_t terms)
{
    for (size_t g = 1; g < (size_t)SCV_BLOCK && terms <= SCV_BLOCK_TERMS_MAX; g *= 4)
        if (terms <= SCV_NOHI_MAX * g) return g;
    if (terms <= SCV_P256_MAX) return SCV_BLOCK;
    return (size_t)SCV_BLOCK * scv_bpr(terms);
}
// Records of slice s (s < P): ceil((terms - s) / P), 0 past the row's end.
inline size_t scv_slice_len(size_t terms, size_t parts, size_t s) { return s < terms ? (terms - s + parts - 1) / parts : 0; }
// Fold steps every lane of a launch walks through: the longest slice's (slice 0).
inline size_t scv_steps(size_t terms, size_t parts) { return (terms + parts - 1) / parts; }
// The longest slice any call can produce: n * terms < 2^31 and SCV_MAX_BPR workgroups per row.
constexpr size_t SCV_LONGEST_SLICE = (SCV_INDEX_LIMIT - 1 + SCV_BLOCK * SCV_MAX_BPR - 1) / (SCV_BLOCK * SCV_MAX_BPR);
// n * terms >= 2^31, without the product
inline bool scv_too_large(size_t n, size_t terms)
{
    return terms != 0 && n >= SCV_INDEX_LIMIT / terms + (SCV_INDEX_LIMIT % terms != 0);
}

enum ScvForm {
    SCV_FORM_BLOCK = 0,      // terms <= SCV_BLOCK_TERMS_MAX: lane t of workgroup g is slice t % P of row g * (SCV_BLOCK / P) + t / P, the tree inside the workgroup
    SCV_FORM_ROW = 1,        // P = SCV_BLOCK: workgroup g is row g
    SCV_FORM_TWO = 2,        // workgroup g holds slices (g % bpr) * SCV_BLOCK ... of row g / bpr and leaves one partial; a second kernel finishes the rows
};
struct ScvPlan {
    size_t parts = 1;        // P
    size_t steps = 0;        // fold steps of the first kernel
    ScvForm form = SCV_FORM_BLOCK;
    size_t rows_per_block = SCV_BLOCK;   // first kernel: rows a workgroup holds (BLOCK), 1 (ROW, TWO)
    size_t blocks_per_row = 1;           // first kernel: workgroups of a row (TWO) = partials the second kernel adds per row
    size_t grid1 = 0;        // workgroups of the first kernel
    size_t grid2 = 0;        // workgroups of the second (one per row), 0: none
    size_t partials = 0;     // partials the first kernel writes into the workspace
    size_t workspace_bytes = 0;
};
// Partial (row i, workgroup b of the row) lies at word (i * blocks_per_row + b) * SCV_PARTIAL_WORDS of the workspace.
inline ScvPlan scv_plan(size_t n, size_t terms)
{
    ScvPlan p;
    p.parts = scv_parts(terms);
    p.steps = scv_steps(terms, p.parts);
    if (terms <= SCV_BLOCK_TERMS_MAX) {
        p.rows_per_block = (size_t)SCV_BLOCK / p.parts;
        p.grid1 = (n + p.rows_per_block - 1) / p.rows_per_block;
        return p;
    }
    p.rows_per_block = 1;
    if (p.parts == (size_t)SCV_BLOCK) {
        p.form = SCV_FORM_ROW;
        p.grid1 = n;
        return p;
    }
    p.form = SCV_FORM_TWO;
    p.blocks_per_row = p.parts / (size_t)SCV_BLOCK;
    p.grid1 = n * p.blocks_per_row;              // <= n * terms / 128 < 2^24
    p.grid2 = n;
    p.partials = p.grid1;
    p.workspace_bytes = p.partials * SCV_PARTIAL_WORDS * sizeof(uint32_t);
    return p;
}
static_assert(SCV_NOHI_MAX * 64 * (SCV_BLOCK / 64) <= SCV_STAGE && SCV_BLOCK_TERMS_MAX <= SCV_STAGE, "a workgroup's block of short rows fits the staging area");

// ---- powers.  Row i is written by a group of G lanes: lane l of the group writes x^l, x^(l + G), ... and steps by x^G, so the
// lanes of a group write consecutive records in every step.  A workgroup keeps up to SCV_POW_STAGE records in LDS and writes them
// out in address order: up to G = 64 (terms <= 4 G) that is its whole contiguous block of 256 / G rows at once; from G = 256 on
// every step of a workgroup is 256 consecutive records and four steps are written out together.
//   terms <=    4: G = 1      <=   16: G = 4      <=   64: G = 16     <=  256: G = 64     <= 16384: G = 256
//   terms <= 262144: G = 4096        above: G = 65536
// G <= max(terms, 1) throughout, so n * G <= n * terms < 2^31.
constexpr size_t SCV_POW_STAGE = 1024;               // records of 40 bytes a workgroup stages
constexpr size_t SCV_POW_STAGE_STEPS = SCV_POW_STAGE / SCV_BLOCK;
constexpr size_t SCV_POW_G256_MAX = 16384;
constexpr size_t SCV_POW_G4096_MAX = 262144;
inline size_t scv_pow_group(size_t terms)
{
    for (size_t g = 1; g < (size_t)SCV_BLOCK; g *= 4)
        if (terms <= SCV_POW_STAGE_STEPS * g) return g;
    if (terms <= SCV_POW_G256_MAX) return 256;
    if (terms <= SCV_POW_G4096_MAX) return 4096;
    return 65536;
}
struct ScvPowPlan {
    size_t group = 1;        // G, a power of two
    size_t steps = 0;        // records a lane writes at most: ceil(terms / G)
    size_t rows_per_block = SCV_BLOCK;   // G < SCV_BLOCK: SCV_BLOCK / G rows side by side; else 1
    size_t blocks_per_row = 1;           // G >= SCV_BLOCK: G / SCV_BLOCK
    size_t grid = 0;
};
inline ScvPowPlan scv_pow_plan(size_t n, size_t terms)
{
    ScvPowPlan p;
    p.group = scv_pow_group(terms);
    p.steps = (terms + p.group - 1) / p.group;
    if (p.group < (size_t)SCV_BLOCK) {
        p.rows_per_block = (size_t)SCV_BLOCK / p.group;
        p.grid = (n + p.rows_per_block - 1) / p.rows_per_block;
    } else {
        p.rows_per_block = 1;
        p.blocks_per_row = p.group / (size_t)SCV_BLOCK;
        p.grid = n * p.blocks_per_row;
    }
    return p;
}
static_assert(SCV_POW_STAGE_STEPS * 64 * (SCV_BLOCK / 64) <= SCV_POW_STAGE, "a workgroup's block of short rows fits the staging area");

}  // namespace zc
