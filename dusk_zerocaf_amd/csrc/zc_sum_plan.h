// zc_sum_plan.h -- what the point sums (zerocaf_hip.hip: zc_ed_sum_rows, zc_ris_sum_rows; kernels in zc_sum.hip.h) derive from
// (n, terms) before they touch the device: the order of association, the kernel form, the grids, how many partials a workgroup
// finishes, the workspace and the index limits.  Plain C++17 without any HIP include: tests/test_sum_rows_plan_emul.py drives
// it on the CPU.  No knob reads into it.
#pragma once
#include <cstddef>
#include <cstdint>

namespace zc {

// The order of association (include/zerocaf_hip_ext_sum_rows.h states it): a row of `terms` points is cut into P = sum_parts(terms)
// slices, slice s holding the points s, s + P, s + 2 P, ...; a slice is folded from the left, and the P partial sums are combined
// by adjacent pairs, level by level.  P = 1 up to SUM_SERIAL_MAX terms; above, the largest power of two that leaves every slice at
// least SUM_MIN_SLICE points, at most SUM_MAX_PARTS.
constexpr size_t SUM_SERIAL_MAX = 32;
constexpr size_t SUM_MIN_SLICE = 16;
constexpr size_t SUM_MAX_PARTS = (size_t)1 << 16;
constexpr int SUM_BLOCK = 256;                       // lanes of a workgroup = the partials one workgroup finishes
constexpr size_t SUM_PARTIAL_WORDS = 40;             // 32-bit words of a partial in the workspace: (Y-X, Y+X, Z, T) of 9 words, the accept bit, 3 unused
constexpr size_t SUM_INDEX_LIMIT = (size_t)1 << 31;  // n * terms stays below this

inline size_t sum_parts(size_t terms)
{
    if (terms <= SUM_SERIAL_MAX) return 1;
    size_t p = 1;
    while (p < SUM_MAX_PARTS && 2 * p * SUM_MIN_SLICE <= terms) p *= 2;
    return p;
}
// Points of slice s (s < P <= terms, or terms == 0): ceil((terms - s) / P).
inline size_t sum_slice_len(size_t terms, size_t parts, size_t s) { return s < terms ? (terms - s + parts - 1) / parts : 0; }
// Fold steps every lane of a launch walks through (the longest slice's, slice 0): ceil(terms / P).
inline size_t sum_steps(size_t terms, size_t parts) { return (terms + parts - 1) / parts; }
// n * terms >= 2^31, without the product
inline bool sum_too_large(size_t n, size_t terms)
{
    return terms != 0 && n >= SUM_INDEX_LIMIT / terms + (SUM_INDEX_LIMIT % terms != 0);
}

enum SumForm {
    SUM_FORM_GROUP = 0,      // P <= SUM_BLOCK: one lane per (row, slice), SUM_BLOCK / P rows per workgroup, the tree inside it; P = 1 is one row per lane
    SUM_FORM_TWO = 1,        // P > SUM_BLOCK: a workgroup per SUM_BLOCK slices leaves one partial, a second kernel finishes a row's P / SUM_BLOCK partials
};
struct SumPlan {
    size_t parts = 1;        // P
    size_t steps = 0;        // fold steps of the first kernel
    SumForm form = SUM_FORM_GROUP;
    size_t rows_per_block = SUM_BLOCK;   // first kernel: rows a workgroup holds (GROUP), 1 (TWO)
    size_t blocks_per_row = 1;           // first kernel: workgroups of a row (TWO) = partials the second kernel finishes per row
    size_t grid1 = 0;        // workgroups of the first kernel
    size_t grid2 = 0;        // workgroups of the second (one per row), 0: none
    size_t partials = 0;     // partials the first kernel writes into the workspace
    size_t workspace_bytes = 0;
};
// Partial (row i, workgroup b of the row) lies at word (i * blocks_per_row + b) * SUM_PARTIAL_WORDS of the workspace.
inline SumPlan sum_plan(size_t n, size_t terms)
{
    SumPlan p;
    p.parts = sum_parts(terms);
    p.steps = sum_steps(terms, p.parts);
    if (p.parts <= (size_t)SUM_BLOCK) {
        p.form = SUM_FORM_GROUP;
        p.rows_per_block = (size_t)SUM_BLOCK / p.parts;
        p.grid1 = (n + p.rows_per_block - 1) / p.rows_per_block;
        return p;
    }
    p.form = SUM_FORM_TWO;
    p.rows_per_block = 1;
    p.blocks_per_row = p.parts / (size_t)SUM_BLOCK;      // <= SUM_MAX_PARTS / SUM_BLOCK = SUM_BLOCK
    p.grid1 = n * p.blocks_per_row;
    p.grid2 = n;
    p.partials = p.grid1;
    p.workspace_bytes = p.partials * SUM_PARTIAL_WORDS * sizeof(uint32_t);
    return p;
}
static_assert(SUM_MAX_PARTS / SUM_BLOCK <= (size_t)SUM_BLOCK, "the second kernel finishes a row's partials in one workgroup");

}  // namespace zc
