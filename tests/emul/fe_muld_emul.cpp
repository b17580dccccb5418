// fe_muld_emul.cpp -- TEST-ONLY host build of fp_mul_d (zc_curve.hip.h), the multiplication by the curve constant d without a
// field multiplication, next to the Montgomery product it replaces, and of the addition formulas that call it.  One call per
// lane, as the kernels make them.  Never shipped.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../dusk_zerocaf_amd/csrc/zc_curve.hip.h"

extern "C" void zc_bound_fail(const char* what, int line)
{
    std::fprintf(stderr, "zc_arith.hip.h / zc_curve.hip.h:%d: bound violated: %s\n", line, what);
    std::abort();
}

using namespace zc;

extern "C" {
// x: n x 9 register limbs as the routine receives them (R-class).  raw: n x 9 limbs of fp_mul_d(x) as they are;
// got / want: n x 5 canonical limbs of fe_store_canon(fp_mul_d(x)) and of fe_store_canon(mont_mul(D_M, x)).
void emul_fe_muld(const u32* x, u32* raw, u64* got, u64* want, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        fe a;
        for (int k = 0; k < 9; k++) a.v[k] = x[9 * i + k];
        const fe r = fp_mul_d(a);
        for (int k = 0; k < 9; k++) raw[9 * i + k] = r.v[k];
        fe_store_canon<FP>(got + 5 * i, r);
        fe_store_canon<FP>(want + 5 * i, mont_mul<FP>(fe_const<FP>(ModP::D_M), a));
    }
}
// the product the routine's result enters: fe_store_canon(mont_mul(fp_mul_d(x), y)) against the two Montgomery products
void emul_fe_muld_times(const u32* x, const u32* y, u64* got, u64* want, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        fe a, b;
        for (int k = 0; k < 9; k++) {
            a.v[k] = x[9 * i + k];
            b.v[k] = y[9 * i + k];
        }
        fe_store_canon<FP>(got + 5 * i, mont_mul<FP>(fp_mul_d(a), b));
        fe_store_canon<FP>(want + 5 * i, mont_mul<FP>(mont_mul<FP>(fe_const<FP>(ModP::D_M), a), b));
    }
}
// p + q for n rows of 20 canonical limbs.  form 0: ptm_add, 1: ptm_add on the independent-chain multiplier, 2: pt_add,
// 3: pt_add on the independent-chain multiplier, 4: pt_add_plain, 5: pt_add_plain on the independent-chain multiplier
void emul_muld_ed_add(const u64* p, const u64* q, u64* out, size_t n, int form)
{
    for (size_t i = 0; i < n; i++) {
        if (form >= 4) {
            const pt a = pt_load_plain(p + 20 * i), b = pt_load_plain(q + 20 * i);
            pt_store_plain(out + 20 * i, form == 5 ? pt_add_plain<true>(a, b) : pt_add_plain<false>(a, b));
            continue;
        }
        const pt a = pt_load(p + 20 * i), b = pt_load(q + 20 * i);
        pt r;
        if (form == 0) r = ptm_to_pt(ptm_add<false>(ptm_from_pt(a), ptm_from_pt(b)));
        else if (form == 1) r = ptm_to_pt(ptm_add<true>(ptm_from_pt(a), ptm_from_pt(b)));
        else if (form == 2) r = pt_add<false>(a, b);
        else r = pt_add<true>(a, b);
        pt_store(out + 20 * i, r);
    }
}
}
