// CPU-tier driver of dusk_zerocaf_amd/csrc/zc_msm_plan.h (tests/test_msm_plan_emul.py): plain g++, no HIP.  For one call of
// one entry point it runs the checks and the plan in the order the host code does and writes every plan field.
#include "../../dusk_zerocaf_amd/csrc/zc_msm_plan.h"

using namespace zc;

// field order of tests/golden/msm_plan_table.json
enum { F_LIMIT, F_BUCKETS, F_C, F_W, F_AFFINE, F_REC, F_T, F_TE, F_SEG, F_M, F_NB, F_NSEG, F_NL0, F_G, F_GW, F_GT = F_GW + 4, F_GSEG = F_GT + 4,
       F_BAD = F_GSEG + 4, F_PASSES, F_PACKED, F_BIG, F_TABLE, F_TILE, F_SORTG, F_NCOLS, F_IDX, F_BITS, F_WS = F_BITS + 4, NF };

static void put_sort(const MsmSortPlan& s, int64_t* o)
{
    o[F_PASSES] = s.passes, o[F_PACKED] = s.packed, o[F_BIG] = s.big, o[F_TABLE] = (int64_t)s.table_words;
    if (s.passes) o[F_TILE] = s.pass[0].tile, o[F_SORTG] = s.pass[0].G, o[F_NCOLS] = s.pass[0].ncols, o[F_IDX] = s.pass[0].idx_bits;
    for (int i = 0; i < s.passes; i++) o[F_BITS + i] = s.pass[i].bits;
}
static void put_plan(const MsmBucketPlan& p, int64_t* o)
{
    o[F_BUCKETS] = p.buckets, o[F_C] = p.c, o[F_W] = p.W, o[F_AFFINE] = p.affine, o[F_REC] = p.rec_bytes, o[F_T] = p.T, o[F_TE] = p.TE, o[F_SEG] = p.seg;
    o[F_M] = (int64_t)p.m, o[F_NB] = (int64_t)p.nb, o[F_NSEG] = (int64_t)p.nseg, o[F_NL0] = (int64_t)p.nl0;
    put_sort(p.sort, o);
}

extern "C" int emul_msm_plan_fields(void) { return NF; }

// kind 0: a zc_msm shard of n pairs (arg: points 16-byte aligned); 1: zc_msm_batch of `batch` >= 2 instances of n pairs (arg: aligned);
// 2: zc_msm_bases_create(n, window_bits = arg) + zc_msm_fixed over `batch` vectors; 3: the sort test hook, n scalars, c = arg.
// knobs: window, affine, ngroups, groups[4], sort_packed, sort_big, sort_g, run, run_edges, seg.  A case past an index limit
// reports the limit alone (as the call fails there); o[F_WS] = bytes of the workspace the call asks for.
extern "C" int emul_msm_plan(int kind, uint64_t n64, uint64_t batch64, int arg, const int32_t* k, int64_t* o)
{
    const size_t n = (size_t)n64, batch = (size_t)batch64;
    MsmKnobs knobs;
    knobs.window = k[0], knobs.affine = k[1], knobs.ngroups = k[2];
    for (int g = 0; g < 4; g++) knobs.groups[g] = k[3 + g];
    knobs.sort_packed = k[7], knobs.sort_big = k[8], knobs.sort_g = k[9], knobs.run = k[10], knobs.run_edges = k[11], knobs.seg = k[12];
    for (int i = 0; i < NF; i++) o[i] = 0;
    switch (kind) {
    case 0: {
        if (n < MSM_BUCKET_MIN_N) return 0;                // scalar multiplications + folds in buffers of their own
        if ((o[F_LIMIT] = msm_index_limit(n, 0, 0))) return 0;
        const MsmPlan p = msm_plan(n, arg != 0, knobs);
        put_plan(p, o);
        o[F_G] = p.G, o[F_BAD] = p.bad_groups;
        for (int g = 0; g < 4; g++) o[F_GW + g] = p.gw[g], o[F_GT + g] = p.gT[g], o[F_GSEG + g] = p.gseg[g];
        if (p.bad_groups || (o[F_LIMIT] = msm_index_limit(0, p.m, 0))) return 0;
        o[F_WS] = (int64_t)msm_workspace_layout(p, n, (size_t)p.G + 1).total;
        return 0;
    }
    case 1: {
        const int c = msm_batch_window_bits(n, knobs);
        const size_t W = (size_t)msm_windows(c), cnt = msm_sat_mul(n, batch);
        if ((o[F_LIMIT] = msm_index_limit(cnt, msm_sat_mul(cnt, W), msm_sat_mul(msm_sat_mul(batch, W), (size_t)1 << (c - 1))))) return 0;
        const MsmBucketPlan p = msm_batch_plan(n, batch, arg != 0, knobs);
        put_plan(p, o);
        const size_t pad = 255;
        o[F_WS] = p.buckets ? (int64_t)msm_workspace_layout(p, cnt, batch).total
                            : (int64_t)(((cnt * 160 + pad) & ~pad) + ((batch * ((n + 1) / 2) * 160 + pad) & ~pad));
        return 0;
    }
    case 2: {
        const int c = arg ? arg : msm_fixed_window_bits(n);
        const size_t W = (size_t)msm_windows(c);
        if ((o[F_LIMIT] = msm_index_limit(msm_sat_mul(n, W), 0, 0))) return 0;
        o[F_C] = c, o[F_W] = (int64_t)W;
        if ((o[F_LIMIT] = msm_index_limit(0, msm_sat_mul(batch, n * W), msm_sat_mul(batch, (size_t)1 << (c - 1))))) return 0;
        const MsmBucketPlan p = msm_fixed_plan(n, c, batch, knobs);
        put_plan(p, o);
        o[F_WS] = (int64_t)msm_workspace_layout(p, 0, 0).total;
        return 0;
    }
    case 3: {
        const int c = arg, W = msm_windows(c);
        if ((o[F_LIMIT] = msm_index_limit(0, msm_sat_mul(n, (size_t)W), 0))) return 0;
        const MsmBucketPlan p = msm_bucket_plan(n, (size_t)W, c, false, knobs);
        o[F_C] = c, o[F_W] = W, o[F_M] = (int64_t)p.m;
        put_sort(p.sort, o);
        o[F_WS] = (int64_t)msm_workspace_layout(p, 0, 0, true).total;
        return 0;
    }
    }
    return 1;
}
