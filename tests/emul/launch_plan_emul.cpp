// CPU-tier driver of dusk_zerocaf_amd/csrc/zc_launch_plan.h (tests/test_launch_plan_emul.py): plain g++, no HIP.  For one
// launch decision of one kind it asks the header as the host code does and writes every field of the answer.
#include "../../dusk_zerocaf_amd/csrc/zc_launch_plan.h"

using namespace zc;

// kind, arguments -> fields (the orders of tests/golden/launch_plan_table.json); returns the number of fields, -1: a malformed case
//   0 host_chunk_elems: cnt, heavy, forced -> chunk
//   1 elementwise_form: cnt, limbs per row, arrays, has a staged kernel, threshold (0: STREAM_BYTES, 1: the point ops'),
//     ZC_TEST_STREAM_MIN_BYTES, all arrays 16-byte aligned -> form, block
//   2 strict_form: cnt, ZC_SCHED=block, =unified, the permutation can be had, CUs, quad_ok -> wants the permutation, its
//     bytes, form, grid
//   3 inversion_form: cnt, in place, ZC_INV_CHUNK, CUs -> form, c, lanes
//   4 ring_plan: slot units, ZC_RING_SLOTS -> units per XCD, slots, rows per launch, table bytes
//   5 lincomb_launch: scalar slots used -> block, LDS bytes
//   6 hash_reader_words: prefix_len, forced to bytes, nparts, the part lengths, the parts' addresses mod 8 -> words
extern "C" int emul_launch_plan(int kind, const int64_t* a, int na, int64_t* o)
{
    switch (kind) {
    case 0:
        if (na != 3) return -1;
        o[0] = (int64_t)host_chunk_elems((size_t)a[0], a[1] != 0, (long)a[2]);
        return 1;
    case 1: {
        if (na != 7) return -1;
        const StagedRule rule = a[4] ? StagedRule{0, ED_STAGED_MIN_POINTS, (unsigned)ZC_BLOCK} : StagedRule{};
        const ElementwiseForm f = elementwise_form((size_t)a[0], (size_t)a[1], (size_t)a[2], a[3] != 0, rule, (long)a[5], a[6] != 0);
        o[0] = f.form, o[1] = f.block;
        return 2;
    }
    case 2: {
        if (na != 6) return -1;
        const size_t cnt = (size_t)a[0];
        const bool wants = strict_wants_permutation(cnt, a[1] != 0);
        const StrictPlan p = strict_form(cnt, a[2] != 0, wants && a[3] != 0, (int)a[4], a[5] != 0);
        o[0] = wants, o[1] = wants ? (int64_t)balance_bytes(cnt) : 0, o[2] = p.form, o[3] = p.grid;
        return 4;
    }
    case 3: {
        if (na != 4) return -1;
        const InversionPlan p = inversion_form((size_t)a[0], a[1] != 0, (long)a[2], (int)a[3]);
        o[0] = p.form, o[1] = (int64_t)p.c, o[2] = (int64_t)p.lanes;
        return 3;
    }
    case 4: {
        if (na != 2 || a[0] < 1) return -1;
        const RingPlan p = ring_plan((size_t)a[0], (unsigned)a[1]);
        o[0] = (int64_t)p.units_per_xcd, o[1] = p.slots, o[2] = (int64_t)p.max_launch, o[3] = (int64_t)p.table_bytes;
        return 4;
    }
    case 5: {
        if (na != 1) return -1;
        const LincombLaunch l = lincomb_launch((size_t)a[0]);
        o[0] = l.block, o[1] = (int64_t)l.lds_bytes;
        return 2;
    }
    case 6: {
        if (na < 3 || a[2] < 1 || a[2] > 4 || na != 3 + 2 * (int)a[2]) return -1;
        size_t len[4];
        unsigned mod8[4];
        for (int j = 0; j < (int)a[2]; j++) len[j] = (size_t)a[3 + j], mod8[j] = (unsigned)a[3 + a[2] + j];
        o[0] = hash_reader_words((size_t)a[0], len, mod8, (size_t)a[2], a[1] != 0);
        return 1;
    }
    }
    return -1;
}
