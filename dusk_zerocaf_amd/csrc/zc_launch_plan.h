// zc_launch_plan.h -- what the row-wise entry points (zerocaf_hip.hip: everything that is not an MSM pipeline) decide on the host
// before they launch: how many rows a host chunk holds, which kernel form a call takes and on what grid, the geometry of the
// windowed core's table ring -- and the constants those decisions share with the kernels (zc_kernels.hip.h includes this file).
// Pure functions of sizes, the knobs of the context's Tuning that a rule reads, the CU count, and alignment / aliasing facts
// passed in as booleans.  Plain C++17 without any HIP include: tests/test_launch_plan_emul.py drives it on the CPU against
// tests/golden/launch_plan_table.json.  zerocaf_hip.hip asks, counts the answer (test-hooks build) and launches what it is told.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "zc_msm_plan.h"      // ZC_BLOCK

namespace zc {

// workgroups of ZC_BLOCK lanes for n lanes
inline unsigned grid_for(size_t n) { return (unsigned)((n + ZC_BLOCK - 1) / ZC_BLOCK); }

// The kernel forms a call can take, one enumerator each (the test-hooks build counts launches per enumerator:
// zc_test_launch_forms).  The values are the form codes of tests/golden/launch_plan_table.json.
enum LaunchForm {
    FORM_PER_LANE = 0,        // element-wise and point ops: every lane reads and writes its own row
    FORM_STAGED,              // ... the workgroup moves its rows through LDS with 16-byte copies
    FORM_STRICT_QUAD,         // strict scalar multiplication: four lanes per row (k_ed_scalar_mul_quad)
    FORM_STRICT_SMALL,        // ... independent column chains (k_ed_scalar_mul_small)
    FORM_STRICT_BLOCK,        // ... one workgroup per 256 rows (k_ed_scalar_mul)
    FORM_STRICT_PW,           // ... persistent waves over the cost-sorted rows (k_ed_scalar_mul_pw)
    FORM_STRICT_PW_UNIFIED,   // ... the same on generic steps only (k_ed_scalar_mul_pw_unified, ZC_SCHED=unified)
    FORM_INV_PER_ELEMENT,     // shared inversions: one element and one inversion per lane
    FORM_INV_CHUNKED,         // ... c elements per lane share one inversion
    FORM_INV_LONE,            // ... the same on the independent-chain multiplier
    LAUNCH_FORMS
};

// ---------------------------------------------------------------- host batches
// Host batches of the long-running kernels (scalar multiplications: >= 10 ms per 2^20 elements)
// move through the device in chunks so that only the first upload and the last download are
// exposed. A chunk is a whole number of full-chip rounds of workgroups (2^17 lanes = 512 blocks),
// otherwise every chunk pays a partially filled tail round: measured on 2^20 strict
// scalar-muls, 4 x 2^18 takes 26.1 ms, 3 chunks 30.2 ms, 1 chunk 32.0 ms (kernel alone 22.5 ms).
// Copy-bound calls (field / point element-wise ops) stay in one piece: pageable copies block the
// calling thread, so chunking them buys no overlap. ZC_HOST_CHUNKS=k forces k chunks.
constexpr size_t CHUNK_ROUND = (size_t)1 << 17;
constexpr size_t MAX_CHUNKS = 4096;
inline size_t host_chunk_elems(size_t cnt, bool heavy, long forced)
{
    size_t chunk = cnt;
    if (forced > 0)
        chunk = (cnt + forced - 1) / forced;
    else if (heavy && cnt >= 4 * CHUNK_ROUND)
        // eight chunks, but none below 2^18 elements: the exposed ends (first upload, last download) shrink with
        // the chunk, the per-chunk launches lose efficiency below 2^18 (2^22 strict scalar-muls: 16 chunks of
        // 2^18 89.4 ms, 8 of 2^19 83.1 ms, 4 of 2^20 85.7 ms; 2^20: 4 chunks of 2^18 23.8 ms, 8 of 2^17 34.8 ms)
        chunk = std::max(2 * CHUNK_ROUND, (cnt / 8 + CHUNK_ROUND - 1) / CHUNK_ROUND * CHUNK_ROUND);
    else if (heavy && cnt >= 2 * CHUNK_ROUND)
        chunk = CHUNK_ROUND;
    chunk = (chunk + 1023) / 1024 * 1024;
    return std::max(chunk, (cnt + MAX_CHUNKS - 1) / MAX_CHUNKS);
}

// ---------------------------------------------------------------- element-wise and point ops
// Streams larger than this (bytes over all arrays of the call) use the LDS-staged kernel
// when one is given: it wins only for the compute-free two-input ops beyond the
// 256 MB Infinity Cache (zc_kernels.hip.h, "LDS-staged element I/O").
constexpr size_t STREAM_BYTES = (size_t)256 << 20;
// The point ops -- 160-byte records, far beyond what a lane reads well on its own -- stage their records ABOVE this many
// points, whatever the number of arrays (below, a launch is a handful of workgroups and the barriers only cost).
constexpr size_t ED_STAGED_MIN_POINTS = (size_t)1 << 12;

// When an op that has a staged kernel takes it: the call's arrays hold more than min_bytes together AND the call has more than
// min_rows rows; `block`: the staged kernel's workgroup size.  The default is the 40-byte element ops'.
struct StagedRule {
    size_t min_bytes = STREAM_BYTES;
    size_t min_rows = 0;
    unsigned block = ZC_BLOCK;
};
struct ElementwiseForm {
    LaunchForm form;          // FORM_PER_LANE or FORM_STAGED
    unsigned block;
};
// A call over `arrays` arrays of cnt rows of limbs_per_row 64-bit limbs.  The staged form needs every array 16-byte aligned.
// test_stream_min (ZC_TEST_STREAM_MIN_BYTES, test-hooks build; 0: not set) lowers STREAM_BYTES itself and no other threshold,
// so that small batches reach the ops staged from there on.
inline ElementwiseForm elementwise_form(size_t cnt, size_t limbs_per_row, size_t arrays, bool has_staged, const StagedRule& rule, long test_stream_min,
                                        bool all_aligned16)
{
    const size_t min_bytes = rule.min_bytes == STREAM_BYTES && test_stream_min > 0 ? (size_t)test_stream_min : rule.min_bytes;
    const bool staged = has_staged && cnt * sizeof(uint64_t) * limbs_per_row * arrays > min_bytes && cnt > rule.min_rows && all_aligned16;
    return staged ? ElementwiseForm{FORM_STAGED, rule.block} : ElementwiseForm{FORM_PER_LANE, (unsigned)ZC_BLOCK};
}

// ---------------------------------------------------------------- strict scalar multiplication
// Cost-sorted permutation for the unified-step kernels (see zc_kernels.hip.h "lane balancing"): natural order for small
// batches, beyond 32-bit row indices or when scratch cannot be had.  The persistent-wave kernel walks it; the block-shaped
// kernels (small batches, ZC_SCHED=block) rank their 256 scalars in LDS instead, which keeps HBM traffic algorithmic.
constexpr size_t BALANCE_MIN_N = 1 << 14;
constexpr int ZC_COST_BINS = 1024;                        // u32 bins of the cost histogram
constexpr size_t BAL_COUNTERS = 64;                       // u32 work counters of the persistent kernels, after the bins
// the balance workspace: the bins, the counters, then one u32 index per row
inline size_t balance_bytes(size_t cnt) { return (ZC_COST_BINS + BAL_COUNTERS + cnt) * sizeof(uint32_t); }
// Strict scalar-mul batches from this size on run on persistent waves over the cost-sorted
// permutation (k_ed_scalar_mul_pw: generic steps alternating with wave-uniform doubling steps); ZC_SCHED=unified keeps the
// persistent waves on generic steps only, ZC_SCHED=block keeps one workgroup per 256 elements.
constexpr size_t PW_MIN_ELEMS = (size_t)1 << 17;
// Launches of at most one workgroup per CU keep a single wave on every SIMD; a lone wave cannot
// hide the latency of the column-ordered multiplier's serial chain, so those launches run the
// variant with independent column chains (2^16 units: 2.09 -> 1.79 ms; from 384 workgroups on the
// default kernel is faster again).
constexpr unsigned SMALL_LAUNCH_BLOCKS = 256;
constexpr size_t QUAD_LAUNCH_ELEMS = (size_t)1 << 14;     // 4 lanes per element still leave one wave per SIMD

// Does a batch of cnt rows ask for the permutation (balance_bytes(cnt) of scratch and three small launches)?
inline bool strict_wants_permutation(size_t cnt, bool sched_block)
{
    return cnt >= PW_MIN_ELEMS && !sched_block && cnt >= BALANCE_MIN_N && cnt <= 0xFFFFFFFFull;
}
struct StrictPlan {
    LaunchForm form;          // FORM_STRICT_*
    unsigned grid;            // workgroups of ZC_BLOCK lanes
};
// The block-shaped kernel of a launch of one workgroup per 256 rows.
inline LaunchForm strict_kernel_for(size_t cnt) { return grid_for(cnt) <= SMALL_LAUNCH_BLOCKS ? FORM_STRICT_SMALL : FORM_STRICT_BLOCK; }
// have_permutation: the batch wanted the permutation and got it; without it a batch of any size falls back to the
// block-shaped kernels.  quad_ok: the call may take four lanes per row (zc_ed_scalar_mul and the small instances of
// zc_msm_batch; the products of a small zc_msm shard stay on one lane per row).
inline StrictPlan strict_form(size_t cnt, bool sched_unified, bool have_permutation, int cus, bool quad_ok = true)
{
    if (have_permutation) return {sched_unified ? FORM_STRICT_PW_UNIFIED : FORM_STRICT_PW, (unsigned)(3 * cus)};
    // four lanes per element: the batch cannot fill the chip anyway, so buy latency with lanes
    if (quad_ok && cnt <= QUAD_LAUNCH_ELEMS) return {FORM_STRICT_QUAD, (unsigned)((cnt + 63) / 64)};
    return {strict_kernel_for(cnt), grid_for(cnt)};
}

// ---------------------------------------------------------------- shared inversions
// Montgomery's trick shares one inversion among the c consecutive elements of a lane (3 multiplications per
// element + one inversion per lane).  c = cnt / INV_LANES_TARGET keeps that many lanes busy, capped at 32;
// below 2 the kernels take one element per lane.  ZC_INV_CHUNK=c (1..64) overrides (tuning, tests).
constexpr size_t INV_LANES_TARGET = 65536;
inline size_t inv_chunk(size_t cnt, long inv_chunk_knob)
{
    if (inv_chunk_knob) return (size_t)inv_chunk_knob;
    size_t c = cnt / INV_LANES_TARGET;
    return c > 32 ? 32 : c;
}
struct InversionPlan {
    LaunchForm form;          // FORM_INV_*
    size_t c;                 // elements per lane (what inv_chunk says, also where one element per lane runs)
    size_t lanes;
};
// An op with one inversion per element: one element per lane for a tiny batch or when the output aliases an input, otherwise
// the chunked kernel -- the lone form, on the independent-chain multiplier, when the lanes leave at most one wave per SIMD
// (2^20 elements: BASELINE configs[1], -7 %).
inline InversionPlan inversion_form(size_t cnt, bool in_place, long inv_chunk_knob, int cus)
{
    const size_t c = inv_chunk(cnt, inv_chunk_knob);
    if (c < 2 || in_place) return {FORM_INV_PER_ELEMENT, c, cnt};
    const size_t lanes = (cnt + c - 1) / c;
    return {lanes <= (size_t)cus * 256 ? FORM_INV_LONE : FORM_INV_CHUNKED, c, lanes};
}

// ---------------------------------------------------------------- the windowed core's table ring
// The windowed-core kernels keep 1 KB of table scratch per lane in a ring of wave slots per XCD
// (zc_kernels.hip.h: ring_acquire / ring_release): 256 MB of tables plus 17 KB of tickets and flags, zeroed
// on the stream before every launch.
constexpr uint32_t RING_XCDS = 8;                      // HW_REG_XCC_ID is masked to this range
constexpr uint32_t RING_SLOTS = 512;                   // wave slots per XCD
constexpr uint32_t RING_TICKET_STRIDE = 32;            // one 128-byte line per XCD's ticket counter
constexpr uint32_t RING_STATE_WORDS = RING_XCDS * RING_TICKET_STRIDE + RING_XCDS * RING_SLOTS;   // zeroed per launch
constexpr uint32_t RING_ERR_WORD = RING_STATE_WORDS;    // behind them (two words, written once by the host): device address of the error word
constexpr uint32_t RING_ALLOC_WORDS = RING_STATE_WORDS + 32;
constexpr uint32_t RING_SLOT_DEAD = 0xFFFFFFFFu;       // flag word of a slot whose queue gave up (a generation count never gets there: < 2^19)
constexpr size_t RING_TABLE_BYTES = (size_t)RING_XCDS * RING_SLOTS * 64 * 1024;
// One launch covers the batch (the kernels index with 32 bits: beyond 2^31 elements the batch goes in pieces, one after
// the other on the stream).  ZC_RING_SLOTS=k (1..512) shrinks the ring so that waves really wait for one another (tests; the
// default leaves more slots than waves fit an XCD).
// zc_ed_lincomb takes `slot_units` consecutive 64 KB units per wave slot, one per term (zc_kernels.hip.h: k_ed_lincomb).
// The table area then grows with the slot, up to LINCOMB_MAX_UNITS units per XCD (1 GB in all): 512 slots up to four terms,
// then 409, 341, 292, 256 for five to eight.  Waves of that kernel resident per XCD: 384 up to five terms, then 320, 320,
// 256 (LDS-bound) -- so the ring has a free slot for every resident wave except at seven terms, where up to 28 waves per
// XCD queue for one (by the ring's own protocol).  The single-unit kernels address the first 256 MB of the area whatever
// its size (their XCD stride stays RING_SLOTS units).
constexpr size_t FAST_MAX_LAUNCH = (size_t)1 << 31;
constexpr size_t LINCOMB_MAX_UNITS = 2048;
inline size_t ring_units_per_xcd(size_t slot_units)
{
    return slot_units <= 1 ? (size_t)RING_SLOTS : std::min((size_t)RING_SLOTS * slot_units, LINCOMB_MAX_UNITS);
}
struct RingPlan {
    size_t units_per_xcd;     // 64 KB units of table per XCD
    uint32_t slots;           // wave slots per XCD this launch hands out
    size_t max_launch;        // rows per launch
    size_t table_bytes;       // the table area over all XCDs
};
inline RingPlan ring_plan(size_t slot_units, unsigned ring_slots_knob)
{
    const size_t units_per_xcd = ring_units_per_xcd(slot_units);
    // a launch hands out fewer than 2^19 generations of its slots (the 19-bit field of the word ring_acquire parks)
    const uint32_t slots = std::min(ring_slots_knob ? (uint32_t)ring_slots_knob : RING_SLOTS, (uint32_t)(units_per_xcd / slot_units));
    return {units_per_xcd, slots, std::min(FAST_MAX_LAUNCH, (size_t)slots << 24), RING_TABLE_BYTES / RING_SLOTS * units_per_xcd};
}
// The lincomb kernels (k_ed_lincomb, k_ris_lincomb) over slots_used scalar slots per row: from five slots on, 128-lane
// workgroups keep a workgroup's LDS (36 bytes per lane and slot) below 37 KB.
struct LincombLaunch {
    unsigned block;
    size_t lds_bytes;
};
inline LincombLaunch lincomb_launch(size_t slots_used)
{
    const unsigned block = slots_used > 4 ? 128u : (unsigned)ZC_BLOCK;
    return {block, 36 * slots_used * block};
}

// ---------------------------------------------------------------- SHA-512 rows
// The word reader takes a message whose prefix and parts are all whole 64-bit words at 8-byte aligned addresses; everything
// else, and every message under ZC_TEST_HASH_READER=bytes (test-hooks build), goes through the byte reader.
inline bool hash_reader_words(size_t prefix_len, const size_t* part_len, const unsigned* ptr_mod8, size_t nparts, bool force_bytes)
{
    bool words = prefix_len % 8 == 0;
    for (size_t j = 0; j < nparts; j++) words = words && part_len[j] % 8 == 0 && ptr_mod8[j] == 0;
    return words && !force_bytes;
}

}  // namespace zc
