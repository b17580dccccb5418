// zc_msm_plan.h -- what the MSM host pipelines (zerocaf_hip.hip: zc_msm, zc_msm_fixed, zc_msm_batch, the sort test hook) derive
// from sizes and knobs before they touch the device: window widths, the key sort's passes, run and segment lengths, window
// groups, the workspace layout, the index limits -- and the constants they share with the kernels (zc_kernels.hip.h includes
// this file).  Plain C++17 without any HIP include: tests/test_msm_plan_emul.py drives it on the CPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>

// Compile-time variants of the MSM pipeline that the plan reads (the others: zc_msm.hip.h; DESIGN-EXPERIMENTS.md has the numbers):
#ifndef ZC_MSM_SEG_QUAD
#define ZC_MSM_SEG_QUAD 16384        // four lanes per segment in launches of at most this many segments (twice as many for the lowest of several window groups)
#endif
#ifndef ZC_MSM_LOW_SEG_HALF
#define ZC_MSM_LOW_SEG_HALF 0        // 1: the lowest window group reduces its buckets in segments of half the length.  Round 6, measured and not
#endif                               // taken: 39 instead of 54 dependent additions, but twice the quads -- k_msm_segments_quad 150 -> 194 us at 2^21 pairs
#ifndef ZC_MSM_GROUP_LANES
#define ZC_MSM_GROUP_LANES 17        // log2 of the lanes a window group's bucket-sum launch keeps busy
#endif
#ifndef ZC_MSM_REC_STRIDE
#define ZC_MSM_REC_STRIDE 128        // stride of the affine records: 128 = one per cache line, 96 = packed (packed 256-bit-word records only)
#endif
// `batch` independent MSMs of n pairs each (zc_msm_batch): instances of at least this many pairs take the bucket regime
// (every instance's windows are sort windows of one key sort; one bucket reduction and one parallel Horner step for all);
// below it, batch n strict scalar multiplications and a pairwise fold per instance.  Sweep at 2^20 pairs in all
// (tools/bench_msm_batch.py --sweep, profiles/r08_msm_batch_sweep.json): see DESIGN.md section 7.2.
#ifndef ZC_MSM_BATCH_BUCKET_MIN_N
#define ZC_MSM_BATCH_BUCKET_MIN_N 64
#endif

namespace zc {

constexpr int ZC_BLOCK = 256;                                  // threads per workgroup of nearly every kernel
constexpr int MSM_SCALAR_BITS = 261;                           // 260-bit limb patterns + the carry of the signed recoding
constexpr int MSM_MIN_C = 5, MSM_MAX_C = 22;
constexpr int MSM_RAW_WORDS = 36;                              // 32-bit words of a bucket / edge record (zc_msm.hip.h)
constexpr int MSM_SORT_PASS_BITS = 9;                          // at most 512 bins per pass (+ 1 in the last)
constexpr int MSM_SORT_KPT = 16;                               // keys per thread and tile of the scatter kernel: tiles of 4096 keys,
constexpr int MSM_SORT_KPT_BIG = 32;                           // or of 8192 (two-word records of large batches: a bin's share of a
                                                               // tile is then a whole 128-byte line even with 512 bins)
constexpr int SCAN_BLOCK_ELEMS = ZC_BLOCK * 16;                // entries per block of the flat scan (zc_sort.hip.h)

struct msm_sort_pass {
    uint32_t n;        // keys per window
    uint32_t W;        // windows
    uint32_t tile;     // keys per tile (256 x keys per thread of the scatter kernel)
    uint32_t G;        // tiles per column
    uint32_t ncols;    // columns per window = ceil(n / (G * TILE))
    uint32_t shift;    // first digit bit of this pass
    uint32_t bits;     // digit bits of this pass
    uint32_t last;     // 1: the pass that takes the top bits (bin = d >> shift, zero digits -> bin 2^bits)
    uint32_t c;        // window width
    uint32_t idx_bits; // PACKED records: bits of the point index field
    uint32_t w0;       // the table's first window (a sort over a GROUP of windows: W of them from w0 on, positions relative to the group's start)
};

// Buckets per reduction segment (one lane each): short segments keep enough lanes busy when there are few
// buckets, long ones spend fewer doublings' worth of work on the (first mod 2^(c-1)) * acc products.
// Measured (2^16 / 2^18 / 2^20 / 2^21 / 2^24 pairs, ms): 8: 1.10 / 1.50 / 2.81 / 4.53 / 24.75,
// 16: 1.17 / 1.55 / 2.77 / 4.42 / 24.40, 32: 1.30 / 1.68 / 2.93 / 4.56 / 24.05.
inline int msm_segment_buckets(size_t nbuckets) { return nbuckets <= ((size_t)1 << 18) ? 8 : nbuckets >= ((size_t)1 << 21) ? 32 : 16; }

// The knobs the plans read: the context's Tuning carries them as its member `msm`, filled from
// the environment when the context is created.  0 / -1 = "not set": the library's own choice applies.
struct MsmKnobs {
    int window = 0;                  // ZC_MSM_WINDOW=c
    int affine = -1;                 // ZC_MSM_AFFINE=0/1: projective 128-byte records / affine 112-byte records whatever the shard size
    int groups[4] = {0, 0, 0, 0};    // ZC_MSM_GROUPS="a,b[,c[,d]]": windows per group, top group first ("1" = one group)
    int ngroups = 0;
    // ---- test-hooks build only
    int sort_packed = -1;            // ZC_MSM_SORT_PACKED=0/1
    int sort_big = -1;               // ZC_MSM_SORT_BIG=0/1
    long sort_g = 0;                 // ZC_MSM_SORT_G=g (1..64)
    int run = 0;                     // ZC_MSM_RUN=T (4..4096)
    int run_edges = 0;               // ZC_MSM_RUN_EDGES=T (4..4096, even)
    int seg = 0;                     // ZC_MSM_SEG=s (power of two, 2..256)
};

// windows of c bits: any 260-bit pattern + the recoding carry
inline int msm_windows(int c) { return (MSM_SCALAR_BITS + c - 1) / c; }

// Window width: signed digits put 2^(c-1) buckets in a window; c = log2(n) - 4 keeps about 32
// points per bucket, where the bucket reduction (~3.7 additions per bucket) stays well below the
// bucket sums (1 addition per point and window); measured flat within 3 % for c +- 1 up to 2^18 and at 2^21,
// and for c = 18..21 at 2^24 (tools/quick_bench.py msmsweep).  ZC_MSM_WINDOW=c overrides (tests, tuning; read at context creation like every knob).
inline int msm_window_bits(size_t cnt, const MsmKnobs& knobs)
{
    int c = 0;
    while (((size_t)1 << (c + 1)) <= cnt) c++;
    c -= 4;
    if (c == 15 || c == 16) c = 17;                       // 2^19, 2^20 pairs: 16 windows of 17 bits beat 18 of 15 / 17 of 16 (measured -4 %)
    if (c < MSM_MIN_C) c = MSM_MIN_C;
    if (c > 18) c = 18;                                   // beyond: no faster (2^24 pairs: c = 18 / 19 / 20: 21.4 / 21.9 / 22.9 ms), bucket memory doubles per step
    if (knobs.window >= MSM_MIN_C && knobs.window <= MSM_MAX_C) c = knobs.window;
    return c;
}
// the width of least cost(c, windows, buckets per window); the narrowest of equals
template <class Cost>
inline int msm_cheapest_window_bits(Cost cost)
{
    int best = MSM_MIN_C;
    double best_cost = 0;
    for (int c = MSM_MIN_C; c <= MSM_MAX_C; c++) {
        const double x = cost((double)msm_windows(c), (double)((size_t)1 << (c - 1)));
        if (c == MSM_MIN_C || x < best_cost) best = c, best_cost = x;
    }
    return best;
}
// Fixed-base table of n bases: per scalar vector the bucket sums cost n W additions and the reduction about 3.7 per
// bucket (the figure behind msm_window_bits), 2^(c-1) buckets: c minimises n ceil(261 / c) + 3.7 2^(c-1).  There is no
// doubling chain to hide, and c is fixed when the table is built.
inline int msm_fixed_window_bits(size_t n)
{
    return msm_cheapest_window_bits([n](double W, double buckets) { return (double)n * W + 3.7 * buckets; });
}
// Batched MSM, bucket regime, per instance: the bucket sums cost n W additions and the reduction about 3.7 per bucket,
// 2^(c-1) buckets per window: c minimises ceil(261 / c) (n + 3.7 2^(c-1)) (about 9 at n = 2^12).  The Horner step's chain is
// shared by all instances, so it does not enter the per-instance cost.  ZC_MSM_WINDOW=c overrides, as for zc_msm.
inline int msm_batch_window_bits(size_t n, const MsmKnobs& knobs)
{
    if (knobs.window >= MSM_MIN_C && knobs.window <= MSM_MAX_C) return knobs.window;
    return msm_cheapest_window_bits([n](double W, double buckets) { return W * ((double)n + 3.7 * buckets); });
}

// The key sort of the MSM (zc_sort.hip.h): `passes` stable counting-sort passes over the c - 1 digit bits of
// every window, at most 9 bits each.  A table column = G tiles of 4096 keys walked by one workgroup of the
// scatter kernel; G grows with the batch so that every window keeps about 128 columns (2^21 pairs per window:
// G = 4; 2^24: G = 16), which bounds the table (windows x bins x columns words) at a few MB.
struct MsmSortPlan {
    int passes = 0;
    bool packed = false;                                      // two passes with the one-word intermediate (zc_sort.hip.h):
                                                              // sign | high digit bits + the zero-digit flag | point index fit 32 bits
    bool big = false;                                         // tiles of 8192 keys
    msm_sort_pass pass[4];
    size_t table_words = 0;                                   // largest table, padded to whole scan blocks
};
// table words of one pass over `nw` windows (a row per window and bin; the last pass's zero digits: a row per window), and
// the same padded to whole scan blocks
inline size_t msm_sort_table_rows(const msm_sort_pass& p, size_t nw) { return (nw * ((size_t)1 << p.bits) + (p.last ? nw : 0)) * p.ncols; }
inline size_t msm_sort_table_words(const msm_sort_pass& p, size_t nw)
{
    return (msm_sort_table_rows(p, nw) + SCAN_BLOCK_ELEMS - 1) / SCAN_BLOCK_ELEMS * SCAN_BLOCK_ELEMS;
}
inline MsmSortPlan msm_sort_plan(size_t n, int c, int W, const MsmKnobs& knobs)
{
    MsmSortPlan pl;
    const int B = c - 1;
    pl.passes = (B + MSM_SORT_PASS_BITS - 1) / MSM_SORT_PASS_BITS;
    // two-word records of large batches: tiles of 8192 keys (ZC_MSM_SORT_BIG=0/1 forces the choice)
    int idx_bits = 1;
    while (((size_t)1 << idx_bits) < n) idx_bits++;
    pl.packed = pl.passes == 2 && 1 + (B - (B + 1) / 2) + 1 + idx_bits <= 32 && knobs.sort_packed != 0;
    pl.big = !pl.packed && n >= ((size_t)1 << 22);
    if (knobs.sort_big >= 0) pl.big = !pl.packed && knobs.sort_big != 0;
    const size_t tile = (size_t)ZC_BLOCK * (pl.big ? MSM_SORT_KPT_BIG : MSM_SORT_KPT);
    const size_t ntiles = (n + tile - 1) / tile;
    size_t G = ntiles / 128;
    G = std::max<size_t>(1, std::min<size_t>(16, G));
    if (knobs.sort_g) G = (size_t)knobs.sort_g;
    const size_t ncols = (ntiles + G - 1) / G;
    int shift = 0;
    for (int i = 0; i < pl.passes; i++) {
        const int bits = B / pl.passes + (i < B % pl.passes ? 1 : 0);
        msm_sort_pass& p = pl.pass[i];
        p.n = (uint32_t)n;
        p.W = (uint32_t)W;
        p.tile = (uint32_t)tile;
        p.G = (uint32_t)G;
        p.ncols = (uint32_t)ncols;
        p.shift = (uint32_t)shift;
        p.bits = (uint32_t)bits;
        p.last = i + 1 == pl.passes ? 1u : 0u;
        p.c = (uint32_t)c;
        p.idx_bits = pl.packed ? (uint32_t)idx_bits : 0;
        p.w0 = 0;
        shift += bits;
        pl.table_words = std::max(pl.table_words, msm_sort_table_words(p, (size_t)W));
    }
    return pl;
}

// ---------------------------------------------------------------- the bucket plans
constexpr size_t MSM_BUCKET_MIN_N = 1 << 12;                  // zc_msm shards below it: n scalar multiplications + pairwise folds
constexpr size_t MSM_BATCH_BUCKET_MIN_N = ZC_MSM_BATCH_BUCKET_MIN_N;
// Affine cached records (7-multiplication bucket additions, 112-byte gathers) from this many points on: the
// normalisation costs one division-step inversion per lane, which small batches cannot amortise.
// ZC_MSM_AFFINE=0/1 forces the choice (tests, A/B).
constexpr size_t MSM_AFFINE_MIN_N = (size_t)1 << 17;
inline bool msm_affine(size_t cnt, const MsmKnobs& knobs) { return knobs.affine >= 0 ? knobs.affine != 0 : cnt >= MSM_AFFINE_MIN_N; }
// Run length of the bucket-sum kernel for a list of m entries: 128 entries per lane, fewer when the list is short (keep
// >= 2^17 lanes = two waves per SIMD busy); longer runs leave fewer edges (2 per run) for the deeper levels.
// Measured (tools/quick_bench.py, ZC_MSM_RUN / ZC_MSM_RUN_EDGES): 2^20 pairs T = 32 / 128 / 256: 2.90 / 2.83 / 3.12 ms;
// 2^21: 4.67 / 4.48 / 4.52; edge runs of 8 / 16 / 32: 2^21 4.44 / 4.53 / 4.63 ms.  Round 3, 2^24 pairs (2^27.9
// entries): T = 128 / 256: 21.94 / 21.53 ms -- half the edges for the deeper levels.
inline int msm_run_length(size_t m, const MsmKnobs& knobs, int lanes_log2 = 17)
{
    if (knobs.run) return knobs.run;                      // T >= 4: every level shortens the list (2 ceil(len / T) < len)
    return m >= ((size_t)1 << 27) ? 256 : (int)std::min<size_t>(128, std::max<size_t>(8, m >> lanes_log2));
}

// One key sort over nw sort windows of n entries each, c-bit digits, and the segmented reduction of its list -- what every
// pipeline derives from its sizes and the knobs.  A sort window is a window of the shard (zc_msm: nw = W, n pairs each), a
// scalar vector of a fixed-base call (n W entries each: the table's records of all windows) or a window of one instance of
// a batch (nw = batch W).
struct MsmBucketPlan {
    bool buckets = false;          // false: the call's small regime -- scalar multiplications + pairwise folds, nothing below applies
    int c = 0, W = 0;              // window bits, windows of a scalar (the batched call reports them in both regimes)
    size_t nw = 0;                 // sort windows
    size_t m = 0, nb = 0;          // list entries (nw n), buckets (nw 2^(c-1): digit magnitudes 1 .. 2^(c-1) per window)
    int T = 0, TE = 8;             // run lengths of the segmented reduction: level 0, deeper levels (short lists, short runs; even: see k_msm_runs_edges)
    int seg = 0;                   // buckets per reduction segment
    size_t nseg = 0, nl0 = 0;      // segments, level-0 lanes
    bool affine = false;           // affine records (27 limb words) + 7-multiplication additions (else 128-byte projective, 8)
    int rec_bytes = 128;           // stride of the cached records (affine: 96 packed or 128 = one per cache line; projective: 128)
    MsmSortPlan sort;
};
inline MsmBucketPlan msm_bucket_plan(size_t n, size_t nw, int c, bool affine, const MsmKnobs& knobs)
{
    MsmBucketPlan p;
    p.buckets = true;
    p.c = c;
    p.W = msm_windows(c);
    p.nw = nw;
    p.m = nw * n;
    p.nb = nw << (c - 1);
    p.sort = msm_sort_plan(n, c, (int)std::min<size_t>(nw, 0x7FFFFFFF), knobs);
    p.T = msm_run_length(p.m, knobs);
    if (knobs.run_edges) p.TE = knobs.run_edges & ~1;
    p.seg = knobs.seg ? knobs.seg : msm_segment_buckets(p.nb);
    while (p.seg > (1 << (c - 1))) p.seg >>= 1;           // a segment never spans windows (ZC_MSM_SEG beside a narrow ZC_MSM_WINDOW)
    p.nseg = p.nb / (size_t)p.seg;
    p.nl0 = (p.m + (size_t)p.T - 1) / (size_t)p.T;
    p.affine = affine;
    // affine records: 108 bytes of payload (rounds 3-5: 96) at a 128-byte stride -- one record per cache line.  Packed (96-byte stride) three records
    // of four straddle two lines: measured (rocprofv3 TCC_EA0_RDREQ of k_msm_runs_affine, profiles/r04_msm_record_stride.md)
    // 34.6 -> 25.1 read requests per pair at 2^21 pairs, 34.3 -> 27.7 at 2^24; 2^21: 3.50 -> 3.50 ms, 2^22: 6.30 -> 6.13, 2^24: 21.18 -> 20.22.
    p.rec_bytes = affine ? ZC_MSM_REC_STRIDE : 128;
    return p;
}
// zc_msm_fixed: the batch's scalar vectors are the sort windows, each n W entries over the table's (affine) records
inline MsmBucketPlan msm_fixed_plan(size_t n, int c, size_t batch, const MsmKnobs& knobs)
{
    return msm_bucket_plan(n * (size_t)msm_windows(c), batch, c, true, knobs);
}
// zc_msm_batch: affine records from batch n >= 2^17 points on, if they are 16-byte aligned (the normalisation's loads)
inline MsmBucketPlan msm_batch_plan(size_t n, size_t batch, bool points_aligned16, const MsmKnobs& knobs)
{
    MsmBucketPlan p;
    if (n == 0 || batch == 0) return p;
    p.c = msm_batch_window_bits(n, knobs);
    p.W = msm_windows(p.c);
    if (n < MSM_BATCH_BUCKET_MIN_N) return p;
    return msm_bucket_plan(n, batch * (size_t)p.W, p.c, msm_affine(batch * n, knobs) && points_aligned16, knobs);
}

// zc_msm's shard: the flat plan over its W windows plus the window groups (zerocaf_hip.hip: msm_on_device), top windows first:
// a bucket-sum launch per group with its own run length; nl0 and nseg are the sums over the groups.  What zc_msm_plan reports.
struct MsmPlan : MsmBucketPlan {
    int G = 1;                     // window groups: gw[g] windows, run length gT[g]
    int gw[4] = {0, 0, 0, 0}, gT[4] = {0, 0, 0, 0};
    int gseg[4] = {0, 0, 0, 0};    // buckets per reduction segment, per group (the lowest group's chain is exposed: shorter segments)
    int bad_groups = 0;            // ZC_MSM_GROUPS was given and adds up to this many windows instead of W: the call fails
};
inline MsmPlan msm_plan(size_t cnt, bool points_aligned16, const MsmKnobs& knobs)
{
    MsmPlan p;
    if (cnt < MSM_BUCKET_MIN_N) return p;
    const int c = msm_window_bits(cnt, knobs);
    // (the normalisation moves the point records with 16-byte loads)
    static_cast<MsmBucketPlan&>(p) = msm_bucket_plan(cnt, (size_t)msm_windows(c), c, msm_affine(cnt, knobs) && points_aligned16, knobs);
    // ZC_MSM_GROUPS="a,b,.." = windows per group, top group first; must add up to W.
    p.gw[0] = p.W;
    {
        int sum = 0;
        for (int g = 0; g < knobs.ngroups; g++) sum += knobs.groups[g];
        if (knobs.ngroups >= 2 && sum == p.W) {
            p.G = knobs.ngroups;
            for (int g = 0; g < p.G; g++) p.gw[g] = knobs.groups[g];
        } else if (knobs.ngroups >= 2) {
            p.bad_groups = sum;                           // fail closed: a split for another window count is not silently replaced by one group
        } else if (knobs.ngroups == 0 && p.W >= 8 && cnt >= ((size_t)1 << 21) && cnt < ((size_t)1 << 22)) {
            // default for config-5-sized shards (2^21 pairs: 16 windows as 9 + 4 + 3): three groups, the lowest (exposed) one the
            // smallest.  Measured on one box, 2^21 pairs (tools/msm_groups_sweep.py): one group 3.68 ms, 13+3 3.50, 12+4 3.51,
            // 10+6 3.74, 7+6+3 3.55, 8+5+3 3.55, 9+4+3 3.44, 6+6+4 3.50, four groups 3.8 - 4.1.  Below 2^21 and from 2^22 on
            // the groups gain nothing (2^20: 2.39 -> 2.59 ms; 2^22: 6.27 -> 6.24; 2^24: 21.2 -> 21.6): one group.
            p.G = 3;
            p.gw[2] = std::max(1, (3 * p.W + 8) / 16);
            p.gw[1] = std::max(1, (4 * p.W + 8) / 16);
            p.gw[0] = p.W - p.gw[1] - p.gw[2];
        }
    }
    // a group's launch keeps 2^17 lanes busy like the whole list (ZC_MSM_GROUP_LANES=16 / 17 / 18 / 19 at 2^21 pairs in three groups:
    // 3.71 / 3.48 / 3.61 / 4.30 ms: shorter runs cut more buckets, and every cut is an edge for the levels behind)
    for (int g = 0; g < p.G; g++)
        p.gT[g] = p.G == 1 ? p.T : msm_run_length(cnt * (size_t)p.gw[g], knobs, ZC_MSM_GROUP_LANES);
    // Segment length per group.  (ZC_MSM_LOW_SEG_HALF: half the length for the lowest group, whose chain is on the call's critical
    // path -- 39 instead of 54 dependent additions; measured in round 6 and not taken, the segments are not pure latency.)
    for (int g = 0; g < p.G; g++) {
        p.gseg[g] = p.seg;
        const size_t nsegg2 = 2 * (size_t)p.gw[g] * (((size_t)1 << (p.c - 1)) / (size_t)p.seg);
        if (ZC_MSM_LOW_SEG_HALF && p.G > 1 && g == p.G - 1 && !knobs.seg && p.seg >= 4 && nsegg2 <= 2 * (size_t)ZC_MSM_SEG_QUAD) p.gseg[g] = p.seg / 2;
    }
    p.nseg = p.nl0 = 0;
    for (int g = 0; g < p.G; g++) {
        p.nseg += (size_t)p.gw[g] * (((size_t)1 << (p.c - 1)) / (size_t)p.gseg[g]);
        p.nl0 += (cnt * (size_t)p.gw[g] + (size_t)p.gT[g] - 1) / (size_t)p.gT[g];   // an upper bound: a group's part of the list is known on the device only
    }
    return p;
}

// ---------------------------------------------------------------- the workspace
// Byte offsets of a call's buffers in the device's one MSM workspace, in this order, each aligned to 256 bytes; `total` is
// what the call needs.  What a call does not use takes no room: pairs_b of a one-pass sort, cached records of a fixed-base
// call (cached_points = 0: the table's), results (out_points = 0: the folded sums are), all behind the sort's part (sort_only).
struct MsmLayout {
    size_t digits = 0, pairs_a = 0, pairs_b = 0, sort_table = 0, sort_sums = 0;     // the key sort: m digit words, m pairs, m pairs or packed words, two tables, the scan's block sums
    size_t cached = 0, buckets = 0, present = 0, ekeys[2] = {0, 0}, erecs[2] = {0, 0};   // 128-byte records, bucket records + flags, edge lists (ping-pong)
    size_t seg_out = 0, fold_b = 0, out = 0;                                          // segment sums and their folds, the call's results (160-byte points)
    size_t total = 0;
};
inline MsmLayout msm_workspace_layout(const MsmBucketPlan& p, size_t cached_points, size_t out_points, bool sort_only = false)
{
    MsmLayout l;
    auto take = [&l](size_t count, size_t elt_bytes) { return std::exchange(l.total, l.total + ((count * elt_bytes + 255) & ~(size_t)255)); };
    l.digits = take(p.m, 4);
    l.pairs_a = take(p.m, 8);
    l.pairs_b = take(p.sort.passes == 1 ? 0 : p.m, p.sort.packed ? 4 : 8);
    l.sort_table = take(2 * p.sort.table_words, 4);
    l.sort_sums = take(p.sort.table_words / SCAN_BLOCK_ELEMS + 1, 4);
    if (sort_only) return l;
    l.cached = take(cached_points * 32, 4);
    l.buckets = take(p.nb * MSM_RAW_WORDS, 4);
    l.present = take(p.nb, 1);
    for (size_t& e : l.ekeys) e = take(2 * p.nl0, 4);
    for (size_t& e : l.erecs) e = take(2 * p.nl0 * MSM_RAW_WORDS, 4);
    l.seg_out = take(p.nseg * 20, 8);
    l.fold_b = take(p.nseg * 20, 8);
    l.out = take(out_points * 20, 8);
    return l;
}

// What the kernels index with, checked before anything is allocated: records (points of a call, a table's records) with
// 31 bits beside the sign, list entries (pairs) and bucket keys with 32.  Products that do not fit size_t saturate.
enum MsmLimit { MSM_LIMIT_OK = 0, MSM_LIMIT_RECORDS = 1, MSM_LIMIT_PAIRS = 2, MSM_LIMIT_KEYS = 3 };
inline size_t msm_sat_mul(size_t a, size_t b) { return b && a > SIZE_MAX / b ? SIZE_MAX : a * b; }
inline MsmLimit msm_index_limit(size_t records, size_t entries, size_t keys)
{
    if (records >= ((size_t)1 << 31)) return MSM_LIMIT_RECORDS;
    if (entries >= ((size_t)1 << 32)) return MSM_LIMIT_PAIRS;
    if (keys >= ((size_t)1 << 32)) return MSM_LIMIT_KEYS;
    return MSM_LIMIT_OK;
}

}  // namespace zc
