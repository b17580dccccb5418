// zerocaf_dlog.hpp -- C++ mirror of include/zerocaf_hip_dlog.h: bounded discrete logs, m with P = m * G and 0 <= m < bound.
//
// A header of its own beside zerocaf.hpp (which it includes): the last step of exponential ElGamal, of a tally, of a Pedersen
// opening with a known blinding.  Same backend, same conventions: a failing status throws std::runtime_error from Backend::check.
// Nothing is constant-time.
#pragma once

#include <optional>
#include <vector>

#include "zerocaf.hpp"
#include "../../include/zerocaf_hip_dlog.h"

namespace zerocaf {

// A baby-step table (zc_dlog_create), freed when the object goes: the 2^bits multiples of G -- of 4 G with coset4, for equality
// modulo E[4], which is what the wire form needs.  A point that is not on the curve or lies in E[8] is refused.  Move-only.
class DlogTable {
public:
    DlogTable(const EdwardsPoint& g, unsigned bits, bool coset4 = false) : bits_(bits), coset4_(coset4)
    {
        uint64_t p[20];
        g.flat(p);
        Backend::check(zc_dlog_create(Backend::ctx(), p, bits, coset4 ? ZC_DLOG_COSET4 : 0u, &id_), "zc_dlog_create");
    }
    DlogTable(const DlogTable&) = delete;
    DlogTable& operator=(const DlogTable&) = delete;
    DlogTable(DlogTable&& o) noexcept : id_(o.id_), bits_(o.bits_), coset4_(o.coset4_) { o.id_ = 0; }
    DlogTable& operator=(DlogTable&& o) noexcept
    {
        if (this != &o) {
            reset();
            id_ = o.id_;
            bits_ = o.bits_;
            coset4_ = o.coset4_;
            o.id_ = 0;
        }
        return *this;
    }
    ~DlogTable() { reset(); }
    unsigned bits() const { return bits_; }
    bool coset4() const { return coset4_; }
    // Row i: m with ps[i] == m * G and m < bound (with coset4: ps[i] - m * G in E[4]), or nothing -- also for a row that is no
    // point of the curve.
    std::vector<std::optional<uint64_t>> ed(const std::vector<EdwardsPoint>& ps, uint64_t bound) const
    {
        std::vector<uint64_t> p(ps.size() * 20), m(ps.size());
        std::vector<uint8_t> found(ps.size());
        for (size_t i = 0; i < ps.size(); i++) ps[i].flat(&p[20 * i]);
        if (!ps.empty()) Backend::check(zc_ed_dlog(Backend::ctx(), id_, p.data(), bound, m.data(), found.data(), nullptr, ps.size()), "zc_ed_dlog");
        return gather(m, found);
    }
    // The same from Ristretto encodings (a coset4 table): nothing for a row that does not decode.
    std::vector<std::optional<uint64_t>> ris(const std::vector<CompressedRistretto>& es, uint64_t bound) const
    {
        std::vector<uint8_t> in(es.size() * 32), found(es.size());
        std::vector<uint64_t> m(es.size());
        for (size_t i = 0; i < es.size(); i++) std::memcpy(&in[32 * i], es[i].bytes.data(), 32);
        if (!es.empty()) Backend::check(zc_ris_dlog(Backend::ctx(), id_, in.data(), bound, m.data(), found.data(), nullptr, es.size()), "zc_ris_dlog");
        return gather(m, found);
    }

private:
    void reset()
    {
        if (id_) zc_dlog_destroy(Backend::ctx(), id_);
        id_ = 0;
    }
    static std::vector<std::optional<uint64_t>> gather(const std::vector<uint64_t>& m, const std::vector<uint8_t>& found)
    {
        std::vector<std::optional<uint64_t>> out(m.size());
        for (size_t i = 0; i < m.size(); i++)
            if (found[i]) out[i] = m[i];
        return out;
    }
    uint64_t id_ = 0;
    unsigned bits_ = 0;
    bool coset4_ = false;
};

}  // namespace zerocaf
