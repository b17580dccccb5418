// scvec_emul.cpp -- TEST-ONLY host build of the device functions behind the scalar vector ops (zc_scvec.hip.h: scv_slice_sum,
// scv_slice_dot, scv_cols_fold, scv_pair, scv_tree_half, scv_b_record, scv_pow_lane; zc_scvec_plan.h: the cut and the grids).  The
// loops stand for the launches: workgroup by workgroup and lane by lane as the kernels place them, the tree level by level, the
// two-kernel form through an array of partials.  What the kernels do beyond that -- the staging through LDS -- is theirs alone.
// A violated bound of the -DZC_CHECK_BOUNDS build is counted, not fatal: emul_scvec_bound_failures().  All memory is the
// caller's, except a shared b, which is copied to the front of a zeroed n x terms array (a planted defect that indexes it by row
// stays inside).  Never shipped.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../dusk_zerocaf_amd/csrc/zc_scvec.hip.h"

static unsigned long long g_bound_failures = 0;
extern "C" void zc_bound_fail(const char* what, int line)
{
    if (!g_bound_failures++) std::fprintf(stderr, "line %d: bound violated: %s\n", line, what);
}

using namespace zc;

namespace {
void take(u64 (&x)[5], const u64* p, bool have)
{
    for (int i = 0; i < 5; i++) x[i] = have ? p[i] : 0;
}
void tree(fe* q, size_t width)
{
    for (size_t w = width; w > 1;) {
        const size_t half = scv_tree_half(w);
        for (size_t s = 0; s < w / 2; s++) q[s] = scv_pair(q[s], q[s + half]);
        w = half;
    }
}
void store(u64* out, const fe& a)
{
    u64 r[5];
    fe_to_limbs52(r, a);
    std::memcpy(out, r, sizeof r);
}
void rows(bool dot, const u64* a, const u64* b, bool shared_b, size_t terms, u64* out, size_t n)
{
    std::vector<u64> padded;
    if (dot && shared_b) {
        padded.assign(5 * n * terms + 5, 0);
        std::memcpy(padded.data(), b, 40 * terms);
        b = padded.data();
    }
    const ScvPlan p = scv_plan(n, terms);
    const bool two = p.form == SCV_FORM_TWO, block = p.form == SCV_FORM_BLOCK;
    const u32 parts = (u32)p.parts, steps = scv_fold_steps((u32)terms, parts);
    const size_t width = block ? p.parts : (size_t)SCV_BLOCK, bpr = p.blocks_per_row;
    std::vector<fe> ws(p.partials), part(SCV_BLOCK);
    for (size_t g = 0; g < p.grid1; g++) {
        const size_t row0 = two ? g / bpr : g * p.rows_per_block, slice0 = two ? (g % bpr) * SCV_BLOCK : 0;
        for (size_t t = 0; t < (size_t)SCV_BLOCK; t++) {
            const size_t row = row0 + t / width, s = slice0 + t % width;
            const bool valid = !block || row < n;
            const auto both = [&](size_t, size_t j, bool have, u64 (&xa)[5], u64 (&xb)[5]) {
                take(xa, have ? a + 5 * (row * terms + j) : nullptr, have);
                take(xb, have && dot ? b + 5 * scv_b_record(shared_b, row, terms, j) : nullptr, have && dot);
            };
            if (block)
                part[t] = dot ? scv_block_slice<true>(valid ? terms : 0, parts, s, steps, both) : scv_block_slice<false>(valid ? terms : 0, parts, s, steps, both);
            else if (dot)
                part[t] = scv_slice_dot(valid ? terms : 0, parts, s, steps, [&](size_t, size_t j, bool have, u64 (&xa)[5], u64 (&xb)[5]) {
                    take(xa, have ? a + 5 * (row * terms + j) : nullptr, have);
                    take(xb, have ? b + 5 * scv_b_record(shared_b, row, terms, j) : nullptr, have);
                });
            else
                part[t] = scv_slice_sum(valid ? terms : 0, parts, s, steps, [&](size_t, size_t j, bool have, u64 (&xa)[5]) { take(xa, have ? a + 5 * (row * terms + j) : nullptr, have); });
        }
        for (size_t base = 0; base < (size_t)SCV_BLOCK; base += width) {
            tree(part.data() + base, width);
            const size_t row = row0 + base / width;
            if (two) ws[g] = part[base];
            else if (row < n) store(out + 5 * row, part[base]);
        }
    }
    for (size_t row = 0; two && row < p.grid2; row++) {
        std::vector<fe> q(SCV_BLOCK, fe_zero());                 // lane t: the partials t, t + 256, ...
        for (size_t e = 0; e < bpr; e++) q[e % SCV_BLOCK] = scv_pair(q[e % SCV_BLOCK], ws[row * bpr + e]);
        tree(q.data(), bpr < (size_t)SCV_BLOCK ? bpr : (size_t)SCV_BLOCK);
        store(out + 5 * row, q[0]);
    }
}
}  // namespace

extern "C" {
unsigned long long emul_scvec_bound_failures() { return g_bound_failures; }
// stage, block_terms_max, p256_max, two_row_terms, max_bpr, carry_every, nohi_max, longest_slice, pow_stage_steps, pow_g256_max, pow_g4096_max
void emul_scvec_constants(unsigned long long* out)
{
    const unsigned long long c[] = {SCV_STAGE, SCV_BLOCK_TERMS_MAX, SCV_P256_MAX, SCV_TWO_ROW_TERMS, SCV_MAX_BPR, SCV_CARRY_EVERY, SCV_NOHI_MAX, SCV_LONGEST_SLICE,
                                    SCV_POW_STAGE_STEPS, SCV_POW_G256_MAX, SCV_POW_G4096_MAX};
    for (int i = 0; i < 11; i++) out[i] = c[i];
}
void emul_sc_sum_rows(const u64* a, size_t terms, u64* out, size_t n) { rows(false, a, nullptr, false, terms, out, n); }
void emul_sc_dot_rows(const u64* a, const u64* b, size_t terms, unsigned flags, u64* out, size_t n) { rows(true, a, b, (flags & 1) != 0, terms, out, n); }
void emul_sc_powers(const u64* x, size_t terms, u64* out, size_t n)
{
    if (terms == 0) return;
    const ScvPowPlan p = scv_pow_plan(n, terms);
    const u32 G = (u32)p.group, steps = scv_fold_steps((u32)terms, G);
    for (size_t g = 0; g < p.grid; g++)
        for (size_t t = 0; t < (size_t)SCV_BLOCK; t++) {
            const bool small = G < (u32)SCV_BLOCK;
            const size_t row = small ? g * p.rows_per_block + t / G : g / p.blocks_per_row;
            const u32 l = small ? (u32)(t % G) : (u32)((g % p.blocks_per_row) * SCV_BLOCK + t);
            const bool valid = row < n;
            u64 xl[5];
            take(xl, valid ? x + 5 * row : nullptr, valid);
            scv_pow_lane(xl, l, G, valid ? (u32)terms : 0, steps, [&](u32, u32 j, bool have, const u64 (&r)[5]) {
                if (have) std::memcpy(out + 5 * (row * terms + j), r, sizeof r);
            });
        }
}
// One slice of m products of the same pair (a, b), as a lane folds it: the longest slices without their memory.
void emul_sc_slice_dot_const(const u64* a, const u64* b, size_t m, u64* out)
{
    store(out, scv_slice_dot(m, 1, 0, m, [&](size_t, size_t, bool have, u64 (&xa)[5], u64 (&xb)[5]) {
        take(xa, a, have);
        take(xb, b, have);
    }));
}
// ... and of m terms of a sum
void emul_sc_slice_sum_const(const u64* a, size_t m, u64* out)
{
    store(out, scv_slice_sum(m, 1, 0, m, [&](size_t, size_t, bool have, u64 (&xa)[5]) { take(xa, a, have); }));
}
}
