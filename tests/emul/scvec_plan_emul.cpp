// scvec_plan_emul.cpp -- TEST-ONLY: dusk_zerocaf_amd/csrc/zc_scvec_plan.h behind a C interface, built with g++ alone (no HIP header
// anywhere).  Never shipped.
#include "../../dusk_zerocaf_amd/csrc/zc_scvec_plan.h"

using namespace zc;

extern "C" {
// block, index_limit, partial_words, stage, block_terms_max, p256_max, two_row_terms, max_bpr, carry_every, nohi_max, longest_slice,
// pow_stage, pow_stage_steps, pow_g256_max, pow_g4096_max
void plan_scvec_constants(unsigned long long* out)
{
    const unsigned long long c[] = {(unsigned long long)SCV_BLOCK, SCV_INDEX_LIMIT, SCV_PARTIAL_WORDS, SCV_STAGE, SCV_BLOCK_TERMS_MAX, SCV_P256_MAX, SCV_TWO_ROW_TERMS, SCV_MAX_BPR,
                                    SCV_CARRY_EVERY, SCV_NOHI_MAX, SCV_LONGEST_SLICE, SCV_POW_STAGE, SCV_POW_STAGE_STEPS, SCV_POW_G256_MAX, SCV_POW_G4096_MAX};
    for (int i = 0; i < 15; i++) out[i] = c[i];
}
int plan_scvec_too_large(unsigned long long n, unsigned long long terms) { return scv_too_large(n, terms); }
unsigned long long plan_scvec_slice_len(unsigned long long terms, unsigned long long parts, unsigned long long s) { return scv_slice_len(terms, parts, s); }
// parts, steps, form, rows_per_block, blocks_per_row, grid1, grid2, partials, workspace_bytes
void plan_scvec(unsigned long long n, unsigned long long terms, unsigned long long* out)
{
    const ScvPlan p = scv_plan(n, terms);
    const unsigned long long c[] = {p.parts, p.steps, (unsigned long long)p.form, p.rows_per_block, p.blocks_per_row, p.grid1, p.grid2, p.partials, p.workspace_bytes};
    for (int i = 0; i < 9; i++) out[i] = c[i];
}
// group, steps, rows_per_block, blocks_per_row, grid
void plan_scvec_pow(unsigned long long n, unsigned long long terms, unsigned long long* out)
{
    const ScvPowPlan p = scv_pow_plan(n, terms);
    const unsigned long long c[] = {p.group, p.steps, p.rows_per_block, p.blocks_per_row, p.grid};
    for (int i = 0; i < 5; i++) out[i] = c[i];
}
}
