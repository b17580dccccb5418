// zerocaf_scvec.hpp -- C++ mirror of include/zerocaf_hip_scvec.h: scalar vector ops mod L -- row sums, inner products and power
// rows.
//
// A header of its own beside zerocaf.hpp (which it includes): the <a, b>, <a, y^n> and y^0 .. y^(n-1) of an inner-product argument,
// the weighted sum of a batch verifier, a Shamir evaluation as a dot product with a power row.  Same backend, same conventions:
// a failing status throws std::runtime_error from Backend::check.  Values are read as sum (w_i mod 2^52) 2^(52 i); every result
// is the canonical residue.  Nothing is constant-time.
#pragma once

#include <stdexcept>
#include <vector>

#include "zerocaf.hpp"
#include "../../include/zerocaf_hip_scvec.h"

namespace zerocaf {

namespace scvec_detail {
// rows of equal length as n * terms * 5 limbs (one spare record, so that data() is never null)
inline std::vector<uint64_t> flat(const std::vector<std::vector<Scalar>>& rows, size_t terms, const char* who)
{
    std::vector<uint64_t> p(rows.size() * terms * 5 + 5);
    for (size_t i = 0; i < rows.size(); i++) {
        if (rows[i].size() != terms) throw std::invalid_argument(std::string(who) + ": rows of different lengths");
        for (size_t j = 0; j < terms; j++) std::memcpy(&p[5 * (i * terms + j)], rows[i][j].l.data(), 40);
    }
    return p;
}
inline std::vector<Scalar> gather(const std::vector<uint64_t>& o, size_t n)
{
    std::vector<Scalar> out(n);
    for (size_t i = 0; i < n; i++) std::memcpy(out[i].l.data(), &o[5 * i], 40);
    return out;
}
}  // namespace scvec_detail

// Row i: rows[i][0] + rows[i][1] + ... mod L.  Every row has the same length; empty rows give zero.
inline std::vector<Scalar> sc_sum_rows(const std::vector<std::vector<Scalar>>& rows)
{
    const size_t n = rows.size(), terms = n ? rows[0].size() : 0;
    const std::vector<uint64_t> a = scvec_detail::flat(rows, terms, "sc_sum_rows");
    std::vector<uint64_t> o(n * 5 + 5);
    if (n) Backend::check(zc_sc_sum_rows(Backend::ctx(), a.data(), terms, o.data(), n), "zc_sc_sum_rows");
    return scvec_detail::gather(o, n);
}
// Row i: sum_j a[i][j] * b[i][j] mod L; a and b have the same shape.
inline std::vector<Scalar> sc_dot_rows(const std::vector<std::vector<Scalar>>& a, const std::vector<std::vector<Scalar>>& b)
{
    const size_t n = a.size(), terms = n ? a[0].size() : 0;
    if (b.size() != n) throw std::invalid_argument("sc_dot_rows: a and b differ in their rows");
    const std::vector<uint64_t> fa = scvec_detail::flat(a, terms, "sc_dot_rows"), fb = scvec_detail::flat(b, terms, "sc_dot_rows");
    std::vector<uint64_t> o(n * 5 + 5);
    if (n) Backend::check(zc_sc_dot_rows(Backend::ctx(), fa.data(), fb.data(), terms, 0u, o.data(), n), "zc_sc_dot_rows");
    return scvec_detail::gather(o, n);
}
// Row i: sum_j a[i][j] * b[j] mod L: one row of b for every row of a (ZC_SC_DOT_SHARED_B) -- weights, Lagrange coefficients, y^n.
inline std::vector<Scalar> sc_dot_rows(const std::vector<std::vector<Scalar>>& a, const std::vector<Scalar>& b)
{
    const size_t n = a.size(), terms = b.size();
    const std::vector<uint64_t> fa = scvec_detail::flat(a, terms, "sc_dot_rows"), fb = scvec_detail::flat({b}, terms, "sc_dot_rows");
    std::vector<uint64_t> o(n * 5 + 5);
    if (n) Backend::check(zc_sc_dot_rows(Backend::ctx(), fa.data(), fb.data(), terms, ZC_SC_DOT_SHARED_B, o.data(), n), "zc_sc_dot_rows");
    return scvec_detail::gather(o, n);
}
// Row i: x[i]^0, x[i]^1, ..., x[i]^(terms - 1) mod L; the first is 1 also for x = 0.
inline std::vector<std::vector<Scalar>> sc_powers(const std::vector<Scalar>& x, size_t terms)
{
    const size_t n = x.size();
    std::vector<uint64_t> fx(n * 5 + 5), o(n * terms * 5 + 5);
    for (size_t i = 0; i < n; i++) std::memcpy(&fx[5 * i], x[i].l.data(), 40);
    if (n && terms) Backend::check(zc_sc_powers(Backend::ctx(), fx.data(), terms, o.data(), n), "zc_sc_powers");
    std::vector<std::vector<Scalar>> out(n, std::vector<Scalar>(terms));
    for (size_t i = 0; i < n; i++)
        for (size_t j = 0; j < terms; j++) std::memcpy(out[i][j].l.data(), &o[5 * (i * terms + j)], 40);
    return out;
}

}  // namespace zerocaf
