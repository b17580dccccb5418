// dlog_emul.cpp -- TEST-ONLY host build of the device functions behind the bounded discrete logs (zc_dlog.hip.h: dlog_setup,
// dlog_build_run, dlog_start, dlog_search; zc_dlog_plan.h: the slot array and the launch slices).  The loops stand for the
// launches: one call of the setup, one call of the builder per lane, one call of the row functions per row and launch (a row
// depends on nothing but itself and the table).  All memory is the caller's.  Never shipped.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../dusk_zerocaf_amd/csrc/zc_dlog.hip.h"

extern "C" void zc_bound_fail(const char* what, int line)
{
    std::fprintf(stderr, "zc_arith.hip.h:%d: bound violated: %s\n", line, what);
    std::abort();
}

using namespace zc;

namespace {
// one launch over n rows, as dlog_rows of zc_dlog.hip.h runs it: W is the launch's offset, `launch` 0 writes the defaults
void launch_rows(int wire, const void* in, size_t n, const u32* setup, const u64* records, const u64* slots, unsigned t, unsigned flags, const dlog_step& W,
                 unsigned launch, u64 first, u64 chunks, u64 bound, u64* m_out, uint8_t* found, uint8_t* ok)
{
    const dlog_table T{records, slots, t};
    const niels S = dlog_niels(dlog_step_load(setup + DLOG_SETUP_STRIDE * DLOG_SETUP_S));
    for (size_t i = 0; i < n; i++) {
        pt P;
        bool good;
        if (wire) {
            u64 w[4];
            std::memcpy(w, static_cast<const uint8_t*>(in) + 32 * i, 32);
            good = ris_decompress(P, w);
        } else {
            good = dlog_load_ed(P, static_cast<const u64*>(in) + 20 * i);
        }
        bool live = good;
        if (launch == 0) {
            m_out[i] = 0;
            found[i] = 0;
            if (ok) ok[i] = good ? 1 : 0;
        } else if (found[i]) {
            live = false;
        }
        P = pt_select(good, P, pt_identity());
        const pt Q = dlog_start(P, (flags & DLOG_FLAG_COSET4) != 0, dlog_niels(W));
        u32 stage[DLOG_STAGE_WORDS];
        u64 m = 0;
        if (dlog_search(m, Q, T, S, first, chunks, bound, live, stage, 1)) {
            m_out[i] = m;
            found[i] = 1;
        }
    }
}
}  // namespace

extern "C" {
// the constants the tests build their rows from
int emul_dlog_chunk() { return DLOG_CHUNK; }
unsigned long long emul_dlog_steps_per_launch() { return DLOG_STEPS_PER_LAUNCH; }
size_t emul_dlog_setup_words() { return DLOG_SETUP_WORDS; }

// k_dlog_setup: the verdict (0 ok, 1 not a point of the curve, 2 generator in E[8]); setup: DLOG_SETUP_WORDS words
unsigned emul_dlog_setup(const u64* point, unsigned t, unsigned flags, u32* setup)
{
    return setup[0] = dlog_setup(setup, point, t, flags);
}
// k_dlog_records: 2^t records of four words
void emul_dlog_records(const u32* setup, unsigned t, u64* records)
{
    for (size_t lane = 0; lane < dlog_build_lanes(t); lane++) {
        u32 stage[DLOG_BUILD_STAGE_WORDS];
        dlog_build_run(records, setup, t, lane, stage, 1);
    }
}
// the host's insertion: the first record that could not be filed, or -1; slots: 2^(t+1) words
long emul_dlog_slots(const u64* records, unsigned t, u64* slots) { return dlog_build_slots(slots, t, records); }
// the record of one point (20 limbs, Z != 0) as the chunk code derives it: a chunk that starts there
void emul_dlog_record(const u64* p, u64* rec)
{
    pt P;
    (void)dlog_load_ed(P, p);
    pt Q = dlog_start(P, false, niels_identity());
    u32 stage[DLOG_BUILD_STAGE_WORDS];
    fe I = dlog_chunk_forward<true>(Q, niels_identity(), stage, 1);
    for (int i = DLOG_CHUNK - 1; i >= 0; i--) {
        u64 w[4];
        dlog_chunk_y<true>(w, I, stage, 1, i);
        w[3] |= dlog_chunk_x_parity(I, stage, 1, i) << 63;
        I = dlog_chunk_back<true>(I, stage, 1, i);
        if (i == 0) std::memcpy(rec, w, 32);
    }
}
// zc_ed_dlog (wire = 0: in = n * 20 limbs) / zc_ris_dlog (wire = 1: in = n * 32 bytes) as the library slices them
void emul_dlog(int wire, const void* in, size_t n, const u32* setup, const u64* records, const u64* slots, unsigned t, unsigned flags, u64 bound,
               u64* m_out, uint8_t* found, uint8_t* ok)
{
    for (u64 k = 0; k < dlog_launches(bound, t); k++) {
        const DlogSlice s = dlog_slice(bound, t, k);
        launch_rows(wire, in, n, setup, records, slots, t, flags, dlog_step_load(setup + dlog_offset_word(k)), (unsigned)k, s.first, s.chunks, bound, m_out, found, ok);
    }
}
// the same search cut at the giant steps cuts[0] = 0 < cuts[1] < ... < cuts[ncuts - 1], multiples of DLOG_CHUNK or not: launch c
// starts from Q_0 + cuts[c] * S, an offset worked out here
void emul_dlog_cut(int wire, const void* in, size_t n, const u32* setup, const u64* records, const u64* slots, unsigned t, unsigned flags, u64 bound,
                   const u64* cuts, size_t ncuts, u64* m_out, uint8_t* found, uint8_t* ok)
{
    const niels S = dlog_niels(dlog_step_load(setup + DLOG_SETUP_STRIDE * DLOG_SETUP_S));
    for (size_t c = 0; c + 1 < ncuts; c++) {
        pt W = pt_identity();
        for (int b = 63; b >= 0; b--) {
            W = pt_add(W, W);
            if ((cuts[c] >> b) & 1) W = pt_add_cached<false, true>(W, S);
        }
        const u64 steps = cuts[c + 1] - cuts[c];
        launch_rows(wire, in, n, setup, records, slots, t, flags, dlog_step_of(dlog_affine(W)), (unsigned)c, cuts[c], (steps + DLOG_CHUNK - 1) / DLOG_CHUNK, bound, m_out, found, ok);
    }
}
}
