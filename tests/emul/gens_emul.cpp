// gens_emul.cpp -- TEST-ONLY host build of the device functions behind the generator sets (zc_gens.hip.h: gens_normalise,
// gens_row_sum; zc_curve.hip.h: comb_table_column, scalar_recode256, base_mul_onto, ris_compress) and, for comparison, of the
// basepoint calls they generalise (base_table_column, scalar_digits256, base_mul).  The loops stand for the launches: a table
// column per call of the builder, one call of the row function per lane (a row depends on nothing but its own scalars and the
// tables).  Tables are the caller's memory: count * 33 * 128 * 32 words.  Never shipped.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../dusk_zerocaf_amd/csrc/zc_gens.hip.h"

extern "C" void zc_bound_fail(const char* what, int line)
{
    std::fprintf(stderr, "zc_arith.hip.h:%d: bound violated: %s\n", line, what);
    std::abort();
}

using namespace zc;

extern "C" {
// k_gens_table_build over `count` workgroups: the first generator that is no point of the curve, or -1; the table of such a
// generator is left as it was
int emul_gens_build(const u64* points, size_t count, u32* tables)
{
    int first_bad = -1;
    for (size_t j = 0; j < count; j++) {
        pt G;
        if (!gens_normalise(G, points + 20 * j)) {
            if (first_bad < 0) first_bad = (int)j;
            continue;
        }
        for (int e = 0; e < ZC_BASE_ENTRIES; e++) comb_table_column(tables + j * GENS_TABLE_WORDS, G, e);
    }
    return first_bad;
}
// k_ed_mul_gens: k n * count * 5, out n * 20
void emul_ed_mul_gens(const u32* tables, size_t count, const u64* k, u64* out, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        u32 rw[9];
        pt_store(out + 20 * i, gens_row_sum(k + 5 * count * i, (int)count, tables, rw, 1, true));
    }
}
// k_ris_mul_gens_compress: out n * 32 bytes
void emul_ris_mul_gens_compress(const u32* tables, size_t count, const u64* k, uint8_t* out, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        u32 rw[9];
        u64 w[4];
        fe_to_words256(w, ris_compress(gens_row_sum(k + 5 * count * i, (int)count, tables, rw, 1, true)));
        std::memcpy(out + 32 * i, w, 32);
    }
}
// k_base_table_build: 33 * 128 * 32 words
void emul_base_table(u32* table)
{
    for (int e = 0; e < ZC_BASE_ENTRIES; e++) base_table_column(table, e);
}
// k_ed_mul_base / k_ris_mul_base_compress on that table, every lane from its own top digit
void emul_ed_mul_base(const u32* table, const u64* k, u64* out, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        u64 l[5];
        load_scalar(l, k + 5 * i);
        int8_t dig[ZC_BASE_WINDOWS];
        const int top = scalar_digits256(dig, 1, l);
        pt_store(out + 20 * i, base_mul(table, dig, 1, top));
    }
}
void emul_ris_mul_base_compress(const u32* table, const u64* k, uint8_t* out, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        u64 l[5], w[4];
        load_scalar(l, k + 5 * i);
        int8_t dig[ZC_BASE_WINDOWS];
        const int top = scalar_digits256(dig, 1, l);
        fe_to_words256(w, ris_compress(base_mul(table, dig, 1, top)));
        std::memcpy(out + 32 * i, w, 32);
    }
}
}
