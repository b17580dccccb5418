"""Catalogue of planted defects for the device arithmetic headers.  Data only: tests/test_mutants_emul.py applies one entry at
a time to a temporary copy of the headers, builds the host emulation from it and requires the named kill-vector family
(tests/kill_vectors.py) to notice.  Nothing here is ever applied to a file of the repository or built for the GPU.

An entry: name, header ("arith" = zc_arith.hip.h, "curve" = zc_curve.hip.h), `old` (occurs exactly once in the header), `new`,
and one of
    family       the kill-vector family that must report at least one failed comparison;
    equivalent   the bound that makes the changed line unobservable, and `survives`: families the changed build must still pass;
    rounds       a shortened inversion schedule: it must be killed by `family` when 30 * rounds < S_MAX (an input of
                 tests/golden/divsteps_worst.json then needs a step the schedule no longer has), and is listed as
                 "not reached, S_max = ..." otherwise -- the search found no input that needs the dropped rounds.
"""

# the largest division-step counts in tests/golden/divsteps_worst.json (checked against the file by the harness)
S_MAX = {"p": 533, "l": 528}

ARITH, CURVE = "arith", "curve"

_TWO_SUBS = ("a value that leaves mont_mul is below T / R + N with T the product of the operands: an operand below 2^260 = R / 2 "
             "against one below x gives less than x / 2 + N.  ")

MUTANTS = [
    # ---------------------------------------------------------------- the inversion schedule
    dict(name="divsteps_19_rounds", header=CURVE, old="for (int round = 0; round < 20; round++) {", new="for (int round = 0; round < 19; round++) {",
         rounds=19, family="longest_inversions_p"),
    dict(name="divsteps_18_rounds", header=CURVE, old="for (int round = 0; round < 20; round++) {", new="for (int round = 0; round < 18; round++) {",
         rounds=18, family="longest_inversions_p"),
    dict(name="divsteps_17_rounds", header=CURVE, old="for (int round = 0; round < 20; round++) {", new="for (int round = 0; round < 17; round++) {",
         rounds=17, family="longest_inversions_p"),
    dict(name="divsteps_17_rounds_mod_l", header=CURVE, old="for (int round = 0; round < 20; round++) {", new="for (int round = 0; round < 17; round++) {",
         rounds=17, family="longest_inversions_l"),
    dict(name="divsteps_final_sign", header=CURVE, old="const int32_t neg = f[8] >> 31;", new="const int32_t neg = 0;", family="field_core"),
    dict(name="update_de_sign_mask_sd", header=CURVE, old="int32_t md = (t.u & sd) + (t.v & se);", new="int32_t md = (t.u & ~sd) + (t.v & se);", family="field_core"),
    # ---------------------------------------------------------------- signs
    dict(name="is_positive_boundary", header=ARITH, old="ZC_DI bool fe_is_positive_canon(const fe& c)\n{\n    u32 borrow = 0;",
         new="ZC_DI bool fe_is_positive_canon(const fe& c)\n{\n    u32 borrow = 1;", family="sign_boundaries"),
    dict(name="words256_is_positive_boundary", header=CURVE, old="    // raw.v[8] holds bits 232..255 (24 bits); HALF[8] = 2^19\n    u32 borrow = 0;",
         new="    // raw.v[8] holds bits 232..255 (24 bits); HALF[8] = 2^19\n    u32 borrow = 1;",
         equivalent="the only input whose answer changes is s = (p - 1) / 2, and ris_decompress -- the one caller -- rejects that encoding whatever "
                    "s_ok says: it decodes to a point with t negative (kill_vectors.ris_class((p - 1) / 2) == 't negative', asserted by the "
                    "sign_boundaries family).  The nearest encodings below it that do decode are in that family.",
         survives=("sign_boundaries", "degenerate_encodings")),
    dict(name="ts_sqrt_of_zero", header=CURVE, old="return t_is_one || t_is_m1 || a_zero;", new="return t_is_one || t_is_m1;", family="sign_boundaries"),
    dict(name="sqrt_ratio_flipped_i", header=CURVE, old="r = fe_select(flipped || flipped_i, ri, r);", new="r = fe_select(flipped, ri, r);", family="field_core"),
    # ---------------------------------------------------------------- codecs
    dict(name="ris_decompress_y_zero", header=CURVE, old="return s_ok && was_sq && t_pos && !y_zero;", new="return s_ok && was_sq && t_pos;", family="degenerate_encodings"),
    dict(name="ris_decompress_t_negative", header=CURVE, old="return s_ok && was_sq && t_pos && !y_zero;", new="return s_ok && was_sq && !y_zero;", family="degenerate_encodings"),
    dict(name="ris_compress_rotate", header=CURVE, old="const fe x = fe_select(rotate, xr, p.X);", new="const fe x = p.X;", family="group_core"),
    dict(name="ris_compress_negy", header=CURVE, old="y = fe_select(negy, fe_reduce<FP>(fp_neg(y)), y);", new="y = fe_select(false, fe_reduce<FP>(fp_neg(y)), y);", family="group_core"),
    dict(name="ris_compress_abs_s", header=CURVE, old="return fe_select(pos, sc, fe_n_minus_canon<FP>(sc));", new="return sc;", family="group_core"),
    dict(name="ed_compress_sign", header=CURVE, old="const bool sign = !fp_eq(fp_mul(r, p.Z), p.X);", new="const bool sign = fp_eq(fp_mul(r, p.Z), p.X);", family="group_core"),
    dict(name="ed_compress_t_is_m1", header=CURVE, old="const fe r = fe_select(t_is_one, x0, fp_mul(x0, fe_const<FP>(ModP::SIX_POW_Q_M)));", new="const fe r = x0;", family="group_core"),
    dict(name="ed_decompress_sign", header=CURVE, old="const fe x = fe_select(sign, fe_reduce<FP>(fp_neg(r)), r);", new="const fe x = r;", family="degenerate_encodings"),
    dict(name="ts_sqrt_ratio_minus_one", header=CURVE, old="    return t_is_one || t_is_m1;\n}\n// Edwards decompress", new="    return t_is_one;\n}\n// Edwards decompress", family="group_core"),
    dict(name="elligator_s_select", header=CURVE, old="s = fe_select(is_sq, s, sp);", new="s = fe_select(true, s, sp);", family="group_core"),
    dict(name="elligator_c_select", header=CURVE, old="const fe c = fe_select(is_sq, minus_one, r);", new="const fe c = minus_one;", family="group_core"),
    dict(name="elligator_sp_sign", header=CURVE, old="sp = fe_select(fp_is_positive(sp), fe_reduce<FP>(fp_neg(sp)), sp);", new="sp = fe_select(!fp_is_positive(sp), fe_reduce<FP>(fp_neg(sp)), sp);", family="group_core"),
    dict(name="ed_is_valid_left", header=CURVE, old="const fe left = fp_mul(fp_sub(ys, xs), zs);", new="const fe left = fp_mul(fe_add(ys, xs), zs);", family="group_core"),
    dict(name="ed_eq_ignores_y", header=CURVE, old="return ex && ey && !fp_is_zero(a.Z) && !fp_is_zero(b.Z);", new="return ex && !fp_is_zero(a.Z) && !fp_is_zero(b.Z);", family="group_core"),
    dict(name="ed_eq_accepts_z_zero", header=CURVE, old="return ex && ey && !fp_is_zero(a.Z) && !fp_is_zero(b.Z);", new="return ex && ey && !fp_is_zero(a.Z);", family="group_core"),
    dict(name="ris_eq_second_identity", header=CURVE, old="return e1 || e2;", new="return e1;", family="group_core"),
    # ---------------------------------------------------------------- zero by value, shared inversions
    dict(name="zero_mod_ignores_top_limb", header=CURVE, old="return (diff | ((u32)t ^ x.v[8])) == 0;", new="return diff == 0;", family="zero_by_value_p"),
    dict(name="zero_mod_ignores_top_limb_mod_l", header=CURVE, old="return (diff | ((u32)t ^ x.v[8])) == 0;", new="return diff == 0;", family="zero_by_value_l"),
    dict(name="zero_mod_ignores_first_limb", header=CURVE, old="diff |= ((u32)t & M29) ^ x.v[i];", new="if (i) diff |= ((u32)t & M29) ^ x.v[i];", family="zero_by_value_p"),
    dict(name="invert_chunk_acc_one_subtraction", header=CURVE, old="fe inv = fe_inverse_divsteps<F>(fe_cond_sub_n<F>(fe_cond_sub_n<F>(acc)));", new="fe inv = fe_inverse_divsteps<F>(fe_cond_sub_n<F>(acc));",
         equivalent=_TWO_SUBS + "acc starts at R mod N < N and every factor is a five-word pattern below 2^260, so acc' < acc / 2 + N: by induction "
                    "acc < 2N for every chunk length, and one subtraction canonicalises it.  [2N, 3N) is unreachable, so there is no row to search for.",
         survives=("zero_by_value_p", "longest_inversions_p", "field_core")),
    dict(name="invert_chunk_res_one_subtraction", header=CURVE, old="fe_to_limbs52(r, fe_cond_sub_n<F>(fe_cond_sub_n<F>(res)));", new="fe_to_limbs52(r, fe_cond_sub_n<F>(res));",
         equivalent=_TWO_SUBS + "inv is canonical (< N) out of the division steps and below 1.5N after each inv * x; the stored prefix is an acc < 2N, so "
                    "res < 1.5N * 2N / R + N < 1.01N.  The division form multiplies a numerator below 2^260 with mont_to(res) < 1.5N: below 1.75N.",
         survives=("zero_by_value_p", "longest_inversions_p", "field_core")),
    # ---------------------------------------------------------------- the stand-alone products
    dict(name="mulmod_two_pass_one_subtraction", header=ARITH, old="fe_to_limbs52(r, fe_cond_sub_n<F>(fe_cond_sub_n<F>(mont_mul<F>(am, fe_from_limbs52(xb)))));",
         new="fe_to_limbs52(r, fe_cond_sub_n<F>(mont_mul<F>(am, fe_from_limbs52(xb))));",
         equivalent=_TWO_SUBS + "am = mont_to(a) = a * RR / R with RR < N: below N / 2 + N = 1.5N; the product with b < 2^260 is below 0.75N + N < 2N.",
         survives=("field_core",)),
    dict(name="sqrmod_two_pass_one_subtraction", header=ARITH, old="fe_to_limbs52(r, fe_cond_sub_n<F>(fe_cond_sub_n<F>(mont_mul<F>(mont_to<F>(a), a))));",
         new="fe_to_limbs52(r, fe_cond_sub_n<F>(mont_mul<F>(mont_to<F>(a), a)));",
         equivalent=_TWO_SUBS + "mont_to(a) < 1.5N and a < 2^260: the product is below 0.75N + N < 2N.", survives=("field_core",)),
    dict(name="mul_one_pass_threshold", header=ARITH, old="mulsq_wave_any((((xa[4] | xb[4]) & M52) >> TOP) != 0)", new="mulsq_wave_any((((xa[4] | xb[4]) & M52) >> (TOP + 1)) != 0)", family="field_core"),
    dict(name="square_one_pass_threshold", header=ARITH, old="mulsq_wave_any(((xa[4] & M52) >> TOP) != 0)", new="mulsq_wave_any(((xa[4] & M52) >> (TOP + 1)) != 0)",
         equivalent="in value, not in its stated bound: an operand a in [2^TOPBIT, 2^(TOPBIT+1)) still fits the square's own scaling (a 2^(S/2) < 2^261), "
                    "X' = a^2 2^S < 2^(2 TOPBIT + 2 + S) gives HI < 2^(TOPBIT+2), |WH| < 2^128 -- wh[4] holds it -- and R' = WLO - WH c 2^S < 2^261 + 2^261 "
                    "< 2 N 2^S, so the one conditional subtraction still canonicalises it; only the asserted bound R' < 1.5 2^261 of a -DZC_CHECK_BOUNDS "
                    "build can be exceeded, and this harness builds without it.  The product's threshold is different: b 2^S no longer "
                    "fits nine limbs (mul_one_pass_threshold, killed).  One bit further the square is wrong in value too (square_one_pass_threshold_two_bits).",
         survives=("field_core",)),
    dict(name="square_one_pass_threshold_two_bits", header=ARITH, old="mulsq_wave_any(((xa[4] & M52) >> TOP) != 0)", new="mulsq_wave_any(((xa[4] & M52) >> (TOP + 2)) != 0)", family="field_core"),
    dict(name="from_limbs52_shl_low_limb", header=ARITH, old="x = (l[0] & M52) << (-bit);", new="x = (l[0] & M52) << (-bit + 1);", family="field_core"),
    dict(name="to_limbs52_shr_offset", header=ARITH, old="const int lo = 29 * k - sh - 52 * j;", new="const int lo = 29 * k + sh - 52 * j;", family="field_core"),
    dict(name="plain_fold_column_range", header=ARITH, old="if (k - i >= 0 && k - i < 5) {\n                col += (i64)(int32_t)x[9 + i]", new="if (k - i >= 0 && k - i < 4) {\n                col += (i64)(int32_t)x[9 + i]", family="field_core"),
    dict(name="plain_fold_wh4_sign", header=ARITH, old="wh[4] = (int32_t)col;", new="wh[4] = -(int32_t)col;", family="field_core"),
    # ---------------------------------------------------------------- limb arithmetic
    dict(name="mont_reduce_cols_limb", header=ARITH, old="t[k + 4] += (u64)m * F::N[4];", new="t[k + 4] += (u64)m * F::N[3];", family="field_core"),
    dict(name="fe_carry_to_7", header=ARITH, old="for (int k = 0; k < 8; k++) {\n        a.v[k + 1] += a.v[k] >> 29;", new="for (int k = 0; k < 7; k++) {\n        a.v[k + 1] += a.v[k] >> 29;",
         family="group_core", canary=True),
    dict(name="fe_carry_mask", header=ARITH, old="a.v[k] &= M29;", new="a.v[k] &= 0x3fffffffu;", family="group_core"),
    dict(name="fe_sub2_second_subtrahend", header=ARITH, old="r.v[i] = a.v[i] + (F::BIAS[i] - b.v[i]) + (F::BIAS[i] - c.v[i]);\n    fe_carry(r);",
         new="r.v[i] = a.v[i] + (F::BIAS[i] - b.v[i]) + (F::BIAS[i] - b.v[i]);\n    fe_carry(r);", family="group_core"),
    dict(name="fe_neg_sign", header=ARITH, old="r.v[i] = F::BIAS[i] - b.v[i];\n    fe_carry(r);", new="r.v[i] = F::BIAS[i] + b.v[i];\n    fe_carry(r);", family="group_core"),
    dict(name="fe_n_minus_canon_borrow", header=ARITH, old="d.v[8] = F::N[8] - c.v[8] - borrow;", new="d.v[8] = F::N[8] - c.v[8];", family="group_core"),
    dict(name="sub_half_parity", header=ARITH, old="const u32 odd = 0u - (r.v[0] & 1u);", new="const u32 odd = 0u;", family="group_core"),
    dict(name="cond_sub_n_equality", header=ARITH, old="const bool neg = (s8 >> 31) != 0;",
         new="const bool neg = (s8 >> 31) != 0 || (d.v[0] | d.v[1] | d.v[2] | d.v[3] | d.v[4] | d.v[5] | d.v[6] | d.v[7] | d.v[8]) == 0;", family="field_core"),
    dict(name="legendre_fallback", header=CURVE, old="if (!done) res = slow;", new="if (!done) res = true;", family="field_core"),
    dict(name="sc_invert_row_zero_flag", header=CURVE, old="*nz = !fe_is_zero_canon(x);", new="*nz = true;", family="field_core"),
    # ---------------------------------------------------------------- scalars for protocols
    dict(name="sc_reduce_wide_constant", header=ARITH, old="fe_const<ModL>(ModL::W256_RR)", new="fe_const<ModL>(ModL::RR)", family="scalar_ext"),
    dict(name="sc_muladd_addend_top_limb", header=ARITH, old="if (k < 9) col += c.v[k];", new="if (k < 8) col += c.v[k];", family="scalar_ext"),
    dict(name="sc_muladd_two_pass_addend", header=ARITH, old="fe s = fe_add(p, mont_mul<F>(fe_from_limbs52(xc), fe_one_m<F>()));", new="fe s = fe_add(p, mont_mul<F>(fe_from_limbs52(xb), fe_one_m<F>()));", family="scalar_ext"),
    # ---------------------------------------------------------------- scalar operands and recodings
    dict(name="scalar_effective_early_stop", header=CURVE, old="l[0] < ((u64)1 << tz);", new="l[0] <= ((u64)1 << tz);", family="group_core"),
    dict(name="scalar_to_words_straddle", header=CURVE, old="if (sh + 32 > 52 && idx + 1 < 5) x |= (l[idx + 1] & M52) << (52 - sh);", new="if (sh + 32 > 52 && idx + 1 < 5) x |= (l[idx + 1] & M52) << (53 - sh);", family="group_core"),
    dict(name="digits16_top_carry", header=CURVE, old="for (int i = 0; i < 66; i++) {", new="for (int i = 0; i < 65; i++) {", family="recoding_fast"),
    dict(name="recode16_top_word", header=CURVE, old="const u32 eights = k < 8 ? 0x88888888u : 0x88u;", new="const u32 eights = k < 8 ? 0x88888888u : 0x08u;", family="recoding_lincomb"),
    dict(name="recode16_carry_between_words", header=CURVE, old="        c += (u64)w[k] + eights;\n        const u32 r = (u32)c;\n        c >>= 32;",
         new="        c += (u64)w[k] + eights;\n        const u32 r = (u32)c;\n        c = 0;", family="recoding_lincomb"),
    dict(name="digits256_top_carry", header=CURVE, old="for (int i = 0; i < ZC_BASE_WINDOWS; i++) {", new="for (int i = 0; i < ZC_BASE_WINDOWS - 1; i++) {", family="recoding_base"),
    dict(name="recode256_top_word", header=CURVE, old="const u32 halves = k < 8 ? 0x80808080u : 0x80u;", new="const u32 halves = k < 8 ? 0x80808080u : 0x00u;", family="recoding_base"),
    dict(name="ltr_digits_bit_248", header=CURVE, old="w[7] &= 0x01FFFFFFu;", new="w[7] &= 0x00FFFFFFu;", family="recoding_fast"),
    dict(name="ltr_digits_naf_length", header=CURVE, old="const bool live = i < 250 &&", new="const bool live = i < 249 &&", family="recoding_fast"),
    # ---------------------------------------------------------------- the strict tile loop
    dict(name="sm_at_top_one_early", header=CURVE, old="return L.active && L.pos >= L.nbits - 1;", new="return L.active && L.pos >= L.nbits - 2;", family="recoding_tile"),
    dict(name="sm_tile_wants_d_step_idle", header=CURVE, old="return any_active && !any_at_top;", new="return !any_at_top;", family="recoding_tile"),
    dict(name="doubling_gate_curve_identity", header=CURVE, old="return fp_eq(rhs, lhs) && fp_eq(mont_mul<FP>(p.T, p.Z), mont_mul<FP>(p.X, p.Y));",
         new="return fp_eq(mont_mul<FP>(p.T, p.Z), mont_mul<FP>(p.X, p.Y));", family="recoding_tile"),
    dict(name="doubling_gate_t_identity", header=CURVE, old="return fp_eq(rhs, lhs) && fp_eq(mont_mul<FP>(p.T, p.Z), mont_mul<FP>(p.X, p.Y));",
         new="return fp_eq(rhs, lhs);", family="recoding_tile"),
    dict(name="ptm_double_valid_f", header=CURVE, old="const fe F = fp_sub(fe_add(D, D), G);", new="const fe F = fp_sub(D, G);", family="recoding_tile"),
    # ---------------------------------------------------------------- cached points
    dict(name="niels_cond_neg_swap", header=CURVE, old="r.ypx = fe_select(neg, q.ymx, q.ypx);", new="r.ypx = q.ypx;", family="group_core"),
    dict(name="niels_cond_neg_t2d", header=CURVE, old="r.t2d = fe_select(neg, fe_neg_lazy<FP>(q.t2d), q.t2d);", new="r.t2d = q.t2d;", family="recoding_fast"),
    dict(name="pt_add_cached_double_z", header=CURVE, old="const fe D = fe_add(ZZ, ZZ);", new="const fe D = ZZ;", family="group_core"),
]
