// zerocaf.hpp -- C++ host-side mirror of zerocaf's operator surface for the hot path,
// over the C ABI of libzerocaf_hip.so (include/zerocaf_hip.h).  Same names, argument
// meaning and error behaviour as the reference's Rust API:
//   FieldElement   src/backend/u64/field.rs  (Add/Sub/Neg/Mul :170-275, Square :302-315,
//                  inverse :854-925 (throws where Rust panics), from_bytes/to_bytes :563-631,
//                  sqrt_ratio_i :462-503, inv_sqrt :443-460)
//   Scalar         src/backend/u64/scalar.rs (Add/Sub/Neg/Mul :139-270, Square :272-283,
//                  from_bytes :445-467 (throws on > L-1), to_bytes :477-516, two_pow_k :525-552)
//   EdwardsPoint   src/edwards.rs (identity :381-391, Neg :440-463, Add :465-501, Sub :503-545,
//                  Mul<Scalar> :547-577, Double :579-592, compress :613-629, == :360-370)
//   CompressedEdwardsY::decompress :313-326 (std::optional = Option)
//   RistrettoPoint / CompressedRistretto  src/ristretto.rs (:96-154, :166-176, :224-425)
//   mul_by_cofactor / mul_by_pow_2  src/edwards.rs:174-191
//   AffinePoint::from :1071-1092, ProjectivePoint add/double/into :809-942/:402-417, is_valid,
//   Elligator / from_uniform_bytes  src/ristretto.rs:430-507; msm / fixed-base batches (not in the reference)
// Single-element operators are batches of one (convenience / tests); use the *_batch
// functions for throughput.  All arithmetic runs on the GPU; there is no CPU path.
#pragma once
#include <array>
#include <cstdint>
#include <cstring>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/zerocaf_hip.h"
#include "../../include/zerocaf_hip_ext.h"

namespace zerocaf {

class Backend {
public:
    static zc_ctx* ctx()
    {
        static Backend b;
        return b.ctx_;
    }
    static void check(int rc, const char* what)
    {
        if (rc != 0) throw std::runtime_error(std::string(what) + " failed: " + zc_last_error());
    }
    static int device_count() { return zc_device_count(); }
    static std::string version() { return zc_version(); }
    // launch on the caller's hipStream_t (device buffers: calls become asynchronous on it) / back to the own stream
    static void set_stream(void* hip_stream) { check(zc_ctx_set_stream(ctx(), hip_stream, 1), "zc_ctx_set_stream"); }
    static void use_own_stream() { check(zc_ctx_set_stream(ctx(), nullptr, 0), "zc_ctx_set_stream"); }
    static void synchronize() { check(zc_ctx_synchronize(ctx()), "zc_ctx_synchronize"); }
    // the HIP device behind slot `slot` of the context (what zc_ctx_create(NULL, 0, ..) picked, or the list it was given)
    static int device(int slot = 0)
    {
        const int d = zc_ctx_device(ctx(), slot);
        if (d < 0) check(d, "zc_ctx_device");
        return d;
    }
    static int slot_count() { return zc_ctx_device_count(ctx()); }
    static void set_stream_dev(int slot, void* hip_stream) { check(zc_ctx_set_stream_dev(ctx(), slot, hip_stream, 1), "zc_ctx_set_stream_dev"); }
    // pin a long-lived host buffer: host batches from it copy asynchronously
    static void host_register(void* p, size_t bytes) { check(zc_host_register(p, bytes), "zc_host_register"); }
    static void host_unregister(void* p) { check(zc_host_unregister(p), "zc_host_unregister"); }
    // one process per GPU: RCCL communicator for the MSM exchange (rank 0 makes the id, every rank joins)
    static std::array<uint8_t, 128> comm_unique_id()
    {
        std::array<uint8_t, 128> id{};
        check(zc_comm_unique_id(id.data()), "zc_comm_unique_id");
        return id;
    }
    static void comm_init(const std::array<uint8_t, 128>& id, int rank, int world) { check(zc_comm_init(ctx(), id.data(), rank, world), "zc_comm_init"); }
    static void comm_destroy() { check(zc_comm_destroy(ctx()), "zc_comm_destroy"); }
    static int comm_size() { int r = 0; check(zc_comm_size(ctx(), &r), "zc_comm_size"); return r; }   // ncclCommCount; 0 without a communicator

private:
    Backend() { check(zc_ctx_create(nullptr, 0, &ctx_), "zc_ctx_create"); }
    ~Backend() { zc_ctx_destroy(ctx_); }
    zc_ctx* ctx_ = nullptr;
};

struct Scalar;

struct FieldElement {
    std::array<uint64_t, 5> l{};
    FieldElement() = default;
    FieldElement(std::array<uint64_t, 5> v) : l(v) {}
    explicit FieldElement(uint64_t v) { l = {v & ((1ull << 52) - 1), v >> 52, 0, 0, 0}; }   // From<u64>, field.rs:124-133
    static FieldElement zero() { return FieldElement(); }
    static FieldElement one() { return FieldElement(std::array<uint64_t, 5>{1, 0, 0, 0, 0}); }
    static FieldElement minus_one() { return FieldElement(std::array<uint64_t, 5>{671914833335276ull, 3916664325105025ull, 1367801ull, 0, 17592186044416ull}); }
    static FieldElement two_pow_k(uint64_t k)                               // field.rs:640-666 (host-side constructor, as in the reference)
    {
        if (k >= 253) throw std::domain_error("Exponent can't be greater than 260");
        FieldElement r;
        r.l[k / 52] = 1ull << (k % 52);
        return r;
    }

    FieldElement operator+(const FieldElement& b) const { FieldElement r; Backend::check(zc_fe_add(Backend::ctx(), l.data(), b.l.data(), r.l.data(), 1), "zc_fe_add"); return r; }
    FieldElement operator-(const FieldElement& b) const { FieldElement r; Backend::check(zc_fe_sub(Backend::ctx(), l.data(), b.l.data(), r.l.data(), 1), "zc_fe_sub"); return r; }
    FieldElement operator*(const FieldElement& b) const { FieldElement r; Backend::check(zc_fe_mul(Backend::ctx(), l.data(), b.l.data(), r.l.data(), 1), "zc_fe_mul"); return r; }
    FieldElement operator-() const { FieldElement r; Backend::check(zc_fe_neg(Backend::ctx(), l.data(), r.l.data(), 1), "zc_fe_neg"); return r; }
    FieldElement square() const { FieldElement r; Backend::check(zc_fe_square(Backend::ctx(), l.data(), r.l.data(), 1), "zc_fe_square"); return r; }
    FieldElement inverse() const
    {
        FieldElement r;
        uint8_t ok = 0;
        Backend::check(zc_fe_invert(Backend::ctx(), l.data(), r.l.data(), &ok, 1), "zc_fe_invert");
        if (!ok) throw std::domain_error("inverse of zero");             // field.rs:864 assert!
        return r;
    }
    FieldElement operator/(const FieldElement& b) const
    {
        FieldElement r;
        uint8_t ok = 0;
        Backend::check(zc_fe_div(Backend::ctx(), l.data(), b.l.data(), r.l.data(), &ok, 1), "zc_fe_div");
        if (!ok) throw std::domain_error("Cannot divide by zero.");           // field.rs:285
        return r;
    }
    FieldElement half() const { FieldElement r; Backend::check(zc_fe_half(Backend::ctx(), l.data(), r.l.data(), 1), "zc_fe_half"); return r; }   // Half, field.rs:317-323
    FieldElement pow(const FieldElement& e) const                                       // Pow, field.rs:325-355
    {
        FieldElement r;
        Backend::check(zc_fe_pow(Backend::ctx(), l.data(), e.l.data(), r.l.data(), 1), "zc_fe_pow");
        return r;
    }
    bool legendre_symbol() const                                                        // field.rs:703-706
    {
        uint8_t c = 0;
        Backend::check(zc_fe_legendre_symbol(Backend::ctx(), l.data(), &c, 1), "zc_fe_legendre_symbol");
        return c != 0;
    }
    bool is_positive() const                                                            // field.rs:552-557
    {
        uint8_t c = 0;
        Backend::check(zc_fe_is_positive(Backend::ctx(), l.data(), &c, 1), "zc_fe_is_positive");
        return c != 0;
    }
    bool is_even() const { return (l[0] & 1) == 0; }                                    // field.rs:534-539
    std::optional<FieldElement> mod_sqrt(bool sign) const;                              // ModSqrt, field.rs:357-441
    // (Choice, FieldElement), field.rs:462-503
    std::pair<bool, FieldElement> sqrt_ratio_i(const FieldElement& v) const
    {
        FieldElement r;
        uint8_t sq = 0;
        Backend::check(zc_fe_sqrt_ratio_i(Backend::ctx(), l.data(), v.l.data(), r.l.data(), &sq, 1), "zc_fe_sqrt_ratio_i");
        return {sq != 0, r};
    }
    std::pair<bool, FieldElement> inv_sqrt() const                                      // InvSqrt, field.rs:443-460
    {
        FieldElement r;
        uint8_t sq = 0;
        Backend::check(zc_fe_inv_sqrt(Backend::ctx(), l.data(), r.l.data(), &sq, 1), "zc_fe_inv_sqrt");
        return {sq != 0, r};
    }
    static FieldElement from_bytes(const std::array<uint8_t, 32>& b)
    {
        FieldElement r;
        Backend::check(zc_fe_from_bytes(Backend::ctx(), b.data(), r.l.data(), 1), "zc_fe_from_bytes");
        return r;
    }
    std::array<uint8_t, 32> to_bytes() const
    {
        std::array<uint8_t, 32> b{};
        Backend::check(zc_fe_to_bytes(Backend::ctx(), l.data(), b.data(), 1), "zc_fe_to_bytes");
        return b;
    }
    bool operator==(const FieldElement& o) const { return to_bytes() == o.to_bytes(); }     // src/field.rs:93-106
    bool operator!=(const FieldElement& o) const { return !(*this == o); }
    uint64_t operator[](size_t i) const { return l[i]; }
};

inline std::optional<FieldElement> FieldElement::mod_sqrt(bool sign) const
{
    FieldElement r;
    uint8_t ok = 0;
    Backend::check(zc_fe_mod_sqrt(Backend::ctx(), l.data(), sign ? 1 : 0, r.l.data(), &ok, 1), "zc_fe_mod_sqrt");
    if (!ok) return std::nullopt;
    return r;
}

struct Scalar {
    std::array<uint64_t, 5> l{};
    Scalar() = default;
    Scalar(std::array<uint64_t, 5> v) : l(v) {}
    explicit Scalar(uint64_t v) { l = {v & ((1ull << 52) - 1), v >> 52, 0, 0, 0}; }
    static Scalar zero() { return Scalar(); }
    static Scalar one() { return Scalar(std::array<uint64_t, 5>{1, 0, 0, 0, 0}); }
    static Scalar minus_one() { return Scalar(std::array<uint64_t, 5>{1129677152307298ull, 1363544697812651ull, 714439ull, 0, 2199023255552ull}); }
    static Scalar two_pow_k(uint64_t k)                                     // scalar.rs:525-552
    {
        if (k >= 250) throw std::domain_error("Exponent can't be greater than the sub-group order");
        Scalar s;
        s.l[k / 52] = 1ull << (k % 52);
        return s;
    }
    Scalar operator+(const Scalar& b) const { Scalar r; Backend::check(zc_sc_add(Backend::ctx(), l.data(), b.l.data(), r.l.data(), 1), "zc_sc_add"); return r; }
    Scalar operator-(const Scalar& b) const { Scalar r; Backend::check(zc_sc_sub(Backend::ctx(), l.data(), b.l.data(), r.l.data(), 1), "zc_sc_sub"); return r; }
    Scalar operator*(const Scalar& b) const { Scalar r; Backend::check(zc_sc_mul(Backend::ctx(), l.data(), b.l.data(), r.l.data(), 1), "zc_sc_mul"); return r; }
    Scalar operator-() const { Scalar r; Backend::check(zc_sc_neg(Backend::ctx(), l.data(), r.l.data(), 1), "zc_sc_neg"); return r; }
    Scalar square() const { Scalar r; Backend::check(zc_sc_square(Backend::ctx(), l.data(), r.l.data(), 1), "zc_sc_square"); return r; }
    Scalar half() const { Scalar r; Backend::check(zc_sc_half(Backend::ctx(), l.data(), r.l.data(), 1), "zc_sc_half"); return r; }   // Half, scalar.rs:285-291
    Scalar pow(const Scalar& e) const { Scalar r; Backend::check(zc_sc_pow(Backend::ctx(), l.data(), e.l.data(), r.l.data(), 1), "zc_sc_pow"); return r; }   // Pow, :300-322
    Scalar operator>>(uint8_t k) const { Scalar r; Backend::check(zc_sc_shr(Backend::ctx(), l.data(), k, r.l.data(), 1), "zc_sc_shr"); return r; }            // Shr<u8>, :165-182
    std::array<uint8_t, 256> into_bits() const                               // scalar.rs:352-366
    {
        std::array<uint8_t, 256> b{};
        Backend::check(zc_sc_into_bits(Backend::ctx(), l.data(), b.data(), 1), "zc_sc_into_bits");
        return b;
    }
    std::array<int8_t, 256> compute_NAF() const                              // scalar.rs:370-389
    {
        std::array<int8_t, 256> d{};
        Backend::check(zc_sc_compute_naf(Backend::ctx(), l.data(), 0, d.data(), 1), "zc_sc_compute_naf");
        return d;
    }
    std::array<int8_t, 256> compute_window_NAF(uint8_t width) const          // scalar.rs:396-415
    {
        std::array<int8_t, 256> d{};
        Backend::check(zc_sc_compute_naf(Backend::ctx(), l.data(), width, d.data(), 1), "zc_sc_compute_naf");
        return d;
    }
    bool is_even() const { return (l[0] & 1) == 0; }                         // scalar.rs:346-348
    Scalar half_without_mod() const                                         // scalar.rs:562-574
    {
        Scalar r = *this;
        uint64_t carry = 0;
        for (int i = 4; i >= 0; i--) {
            r.l[i] |= carry;
            carry = (r.l[i] & 1) << 52;
            r.l[i] >>= 1;
        }
        return r;
    }
    static Scalar from_bytes(const std::array<uint8_t, 32>& b)
    {
        Scalar r;
        uint8_t ok = 0;
        Backend::check(zc_sc_from_bytes(Backend::ctx(), b.data(), r.l.data(), &ok, 1), "zc_sc_from_bytes");
        if (!ok) throw std::domain_error("scalar bytes > L - 1");            // scalar.rs:465 assert!
        return r;
    }
    // Scalar operations for protocols (not in the reference): every input is accepted, results are canonical
    static Scalar from_bytes_wide(const std::array<uint8_t, 64>& b)          // the 512-bit little-endian integer mod L
    {
        Scalar r;
        Backend::check(zc_sc_from_bytes_wide(Backend::ctx(), b.data(), r.l.data(), 1), "zc_sc_from_bytes_wide");
        return r;
    }
    static Scalar from_bytes_mod_order(const std::array<uint8_t, 32>& b)     // any 32 bytes mod L
    {
        Scalar r;
        Backend::check(zc_sc_from_bytes_mod_order(Backend::ctx(), b.data(), r.l.data(), 1), "zc_sc_from_bytes_mod_order");
        return r;
    }
    Scalar muladd(const Scalar& b, const Scalar& c) const                    // *this * b + c
    {
        Scalar r;
        Backend::check(zc_sc_muladd(Backend::ctx(), l.data(), b.l.data(), c.l.data(), r.l.data(), 1), "zc_sc_muladd");
        return r;
    }
    Scalar invert() const                                                    // a^-1 mod L; a = 0 mod L (by value) throws
    {
        Scalar r;
        uint8_t ok = 0;
        Backend::check(zc_sc_invert(Backend::ctx(), l.data(), r.l.data(), &ok, 1), "zc_sc_invert");
        if (!ok) throw std::domain_error("scalar is 0 mod L: no inverse");
        return r;
    }
    std::array<uint8_t, 32> to_bytes() const
    {
        std::array<uint8_t, 32> b{};
        Backend::check(zc_sc_to_bytes(Backend::ctx(), l.data(), b.data(), 1), "zc_sc_to_bytes");
        return b;
    }
    bool operator==(const Scalar& o) const { return to_bytes() == o.to_bytes(); }           // src/scalar.rs:78-91
    uint64_t operator[](size_t i) const { return l[i]; }
};

struct CompressedEdwardsY;
struct CompressedRistretto;

struct EdwardsPoint {
    FieldElement X, Y, Z, T;
    static EdwardsPoint identity() { return {FieldElement::zero(), FieldElement::one(), FieldElement::one(), FieldElement::zero()}; }
    void flat(uint64_t* o) const
    {
        std::memcpy(o, X.l.data(), 40);
        std::memcpy(o + 5, Y.l.data(), 40);
        std::memcpy(o + 10, Z.l.data(), 40);
        std::memcpy(o + 15, T.l.data(), 40);
    }
    static EdwardsPoint unflat(const uint64_t* p)
    {
        EdwardsPoint r;
        std::memcpy(r.X.l.data(), p, 40);
        std::memcpy(r.Y.l.data(), p + 5, 40);
        std::memcpy(r.Z.l.data(), p + 10, 40);
        std::memcpy(r.T.l.data(), p + 15, 40);
        return r;
    }
    EdwardsPoint operator+(const EdwardsPoint& q) const
    {
        uint64_t a[20], b[20], o[20];
        flat(a); q.flat(b);
        Backend::check(zc_ed_add(Backend::ctx(), a, b, o, 1), "zc_ed_add");
        return unflat(o);
    }
    EdwardsPoint operator-(const EdwardsPoint& q) const
    {
        uint64_t a[20], b[20], o[20];
        flat(a); q.flat(b);
        Backend::check(zc_ed_sub(Backend::ctx(), a, b, o, 1), "zc_ed_sub");
        return unflat(o);
    }
    EdwardsPoint operator-() const
    {
        uint64_t a[20], o[20];
        flat(a);
        Backend::check(zc_ed_neg(Backend::ctx(), a, o, 1), "zc_ed_neg");
        return unflat(o);
    }
    EdwardsPoint double_() const
    {
        uint64_t a[20], o[20];
        flat(a);
        Backend::check(zc_ed_double(Backend::ctx(), a, o, 1), "zc_ed_double");
        return unflat(o);
    }
    EdwardsPoint operator*(const Scalar& k) const                           // double_and_add, edwards.rs:102-120
    {
        uint64_t a[20], o[20];
        flat(a);
        Backend::check(zc_ed_scalar_mul(Backend::ctx(), a, k.l.data(), o, 1, ZC_SCALAR_MUL_STRICT), "zc_ed_scalar_mul");
        return unflat(o);
    }
    bool operator==(const EdwardsPoint& q) const                            // affine equality, edwards.rs:360-370
    {
        uint64_t a[20], b[20];
        uint8_t e = 0;
        flat(a); q.flat(b);
        Backend::check(zc_ed_eq(Backend::ctx(), a, b, &e, 1), "zc_ed_eq");
        return e != 0;
    }
    bool is_valid() const                                                   // ValidityCheck, edwards.rs:393-400
    {
        uint64_t a[20];
        uint8_t v = 0;
        flat(a);
        Backend::check(zc_ed_is_valid(Backend::ctx(), a, &v, 1), "zc_ed_is_valid");
        return v != 0;
    }
    inline CompressedEdwardsY compress() const;
};

// AffinePoint::from(EdwardsPoint), edwards.rs:1071-1092 (throws where the inverse of Z = 0 panics)
struct AffinePoint {
    FieldElement X, Y;
    static AffinePoint from(const EdwardsPoint& p)
    {
        uint64_t a[20], xy[10];
        uint8_t ok = 0;
        p.flat(a);
        Backend::check(zc_ed_to_affine(Backend::ctx(), a, xy, &ok, 1), "zc_ed_to_affine");
        if (!ok) throw std::domain_error("inverse of zero");
        AffinePoint r;
        std::memcpy(r.X.l.data(), xy, 40);
        std::memcpy(r.Y.l.data(), xy + 5, 40);
        return r;
    }
};

// ProjectivePoint (edwards.rs:666-998): add :809-865, double :905-942, into EdwardsPoint :402-417
struct ProjectivePoint {
    FieldElement X, Y, Z;
    void flat(uint64_t* o) const
    {
        std::memcpy(o, X.l.data(), 40);
        std::memcpy(o + 5, Y.l.data(), 40);
        std::memcpy(o + 10, Z.l.data(), 40);
    }
    static ProjectivePoint unflat(const uint64_t* p)
    {
        ProjectivePoint r;
        std::memcpy(r.X.l.data(), p, 40);
        std::memcpy(r.Y.l.data(), p + 5, 40);
        std::memcpy(r.Z.l.data(), p + 10, 40);
        return r;
    }
    ProjectivePoint operator+(const ProjectivePoint& q) const
    {
        uint64_t a[15], b[15], o[15];
        flat(a); q.flat(b);
        Backend::check(zc_proj_add(Backend::ctx(), a, b, o, 1), "zc_proj_add");
        return unflat(o);
    }
    ProjectivePoint double_() const
    {
        uint64_t a[15], o[15];
        flat(a);
        Backend::check(zc_proj_double(Backend::ctx(), a, o, 1), "zc_proj_double");
        return unflat(o);
    }
    EdwardsPoint to_extended() const
    {
        uint64_t a[15], o[20];
        flat(a);
        Backend::check(zc_proj_to_extended(Backend::ctx(), a, o, 1), "zc_proj_to_extended");
        return EdwardsPoint::unflat(o);
    }
    static ProjectivePoint identity() { ProjectivePoint r; r.Y.l[0] = 1; r.Z.l[0] = 1; return r; }   // edwards.rs:722-731
    ProjectivePoint operator-() const                                       // Neg, edwards.rs:787-807
    {
        uint64_t a[15], o[15];
        flat(a);
        Backend::check(zc_proj_neg(Backend::ctx(), a, o, 1), "zc_proj_neg");
        return unflat(o);
    }
    ProjectivePoint operator-(const ProjectivePoint& q) const               // Sub, edwards.rs:851-879
    {
        uint64_t a[15], b[15], o[15];
        flat(a); q.flat(b);
        Backend::check(zc_proj_sub(Backend::ctx(), a, b, o, 1), "zc_proj_sub");
        return unflat(o);
    }
    ProjectivePoint operator*(const Scalar& k) const                        // Mul<Scalar>, edwards.rs:881-912
    {
        uint64_t a[15], o[15];
        flat(a);
        Backend::check(zc_proj_scalar_mul(Backend::ctx(), a, k.l.data(), o, 1), "zc_proj_scalar_mul");
        return unflat(o);
    }
    bool operator==(const ProjectivePoint& q) const                         // edwards.rs:701-711
    {
        uint64_t a[15], b[15];
        uint8_t e = 0;
        flat(a); q.flat(b);
        Backend::check(zc_proj_eq(Backend::ctx(), a, b, &e, 1), "zc_proj_eq");
        return e != 0;
    }
    bool is_valid() const                                                   // edwards.rs:733-748
    {
        uint64_t a[15];
        uint8_t v = 0;
        flat(a);
        Backend::check(zc_proj_is_valid(Backend::ctx(), a, &v, 1), "zc_proj_is_valid");
        return v != 0;
    }
};
inline std::array<EdwardsPoint, 4> coset4(const EdwardsPoint& p)             // EdwardsPoint::coset4, edwards.rs:603-610
{
    uint64_t a[20], o[80];
    p.flat(a);
    Backend::check(zc_ed_coset4(Backend::ctx(), a, o, 1), "zc_ed_coset4");
    return {EdwardsPoint::unflat(o), EdwardsPoint::unflat(o + 20), EdwardsPoint::unflat(o + 40), EdwardsPoint::unflat(o + 60)};
}

struct CompressedEdwardsY {
    std::array<uint8_t, 32> bytes{};
    static CompressedEdwardsY identity() { CompressedEdwardsY c; c.bytes[0] = 1; return c; }   // edwards.rs:273-283
    std::optional<EdwardsPoint> decompress() const                          // edwards.rs:313-326
    {
        uint64_t o[20];
        uint8_t ok = 0;
        Backend::check(zc_ed_decompress(Backend::ctx(), bytes.data(), o, &ok, 1), "zc_ed_decompress");
        if (!ok) return std::nullopt;
        return EdwardsPoint::unflat(o);
    }
    bool operator==(const CompressedEdwardsY& o) const { return bytes == o.bytes; }
};
inline CompressedEdwardsY EdwardsPoint::compress() const                    // edwards.rs:613-629
{
    uint64_t a[20];
    CompressedEdwardsY c;
    uint8_t ok = 0;
    flat(a);
    Backend::check(zc_ed_compress(Backend::ctx(), a, c.bytes.data(), &ok, 1), "zc_ed_compress");
    if (!ok) throw std::domain_error("compress: point has no affine form / x^2 is not a square");   // unwrap()/assert! panics
    return c;
}

inline EdwardsPoint mul_by_pow_2(const EdwardsPoint& p, uint64_t k)         // edwards.rs:186-191
{
    uint64_t a[20], o[20];
    p.flat(a);
    Backend::check(zc_ed_mul_by_pow_2(Backend::ctx(), a, k, o, 1), "zc_ed_mul_by_pow_2");
    return EdwardsPoint::unflat(o);
}
inline EdwardsPoint mul_by_cofactor(const EdwardsPoint& p)                  // edwards.rs:174-179
{
    uint64_t a[20], o[20];
    p.flat(a);
    Backend::check(zc_ed_mul_by_cofactor(Backend::ctx(), a, o, 1), "zc_ed_mul_by_cofactor");
    return EdwardsPoint::unflat(o);
}

struct RistrettoPoint {
    EdwardsPoint p;                                                         // RistrettoPoint(pub EdwardsPoint)
    static RistrettoPoint identity() { return {EdwardsPoint::identity()}; }
    RistrettoPoint operator+(const RistrettoPoint& q) const { return {p + q.p}; }
    RistrettoPoint operator-(const RistrettoPoint& q) const { return {p + (-q.p)}; }        // ristretto.rs:291-293
    RistrettoPoint operator-() const { return {-p}; }
    RistrettoPoint double_() const { return {p.double_()}; }
    RistrettoPoint operator*(const Scalar& k) const { return {p * k}; }
    bool operator==(const RistrettoPoint& q) const                          // ristretto.rs:166-176
    {
        uint64_t a[20], b[20];
        uint8_t e = 0;
        p.flat(a); q.p.flat(b);
        Backend::check(zc_ris_eq(Backend::ctx(), a, b, &e, 1), "zc_ris_eq");
        return e != 0;
    }
    bool is_valid() const                                                   // ristretto.rs:205-222
    {
        uint64_t a[20];
        uint8_t v = 0;
        p.flat(a);
        Backend::check(zc_ris_is_valid(Backend::ctx(), a, &v, 1), "zc_ris_is_valid");
        return v != 0;
    }
    static RistrettoPoint elligator_ristretto_flavor(const FieldElement& r0)   // ristretto.rs:430-471
    {
        uint64_t o[20];
        Backend::check(zc_ris_elligator(Backend::ctx(), r0.l.data(), o, 1), "zc_ris_elligator");
        return {EdwardsPoint::unflat(o)};
    }
    static RistrettoPoint from_uniform_bytes(const std::array<uint8_t, 64>& b)   // ristretto.rs:493-507
    {
        uint64_t o[20];
        Backend::check(zc_ris_from_uniform_bytes(Backend::ctx(), b.data(), o, 1), "zc_ris_from_uniform_bytes");
        return {EdwardsPoint::unflat(o)};
    }
    inline CompressedRistretto compress() const;
};
struct CompressedRistretto {
    std::array<uint8_t, 32> bytes{};
    static CompressedRistretto identity() { return {}; }
    std::optional<RistrettoPoint> decompress() const                        // ristretto.rs:96-154
    {
        uint64_t o[20];
        uint8_t ok = 0;
        Backend::check(zc_ris_decompress(Backend::ctx(), bytes.data(), o, &ok, 1), "zc_ris_decompress");
        if (!ok) return std::nullopt;
        return RistrettoPoint{EdwardsPoint::unflat(o)};
    }
    bool operator==(const CompressedRistretto& o) const { return bytes == o.bytes; }
};
inline CompressedRistretto RistrettoPoint::compress() const                 // ristretto.rs:398-425
{
    uint64_t a[20];
    CompressedRistretto c;
    p.flat(a);
    Backend::check(zc_ris_compress(Backend::ctx(), a, c.bytes.data(), 1), "zc_ris_compress");
    return c;
}
inline RistrettoPoint operator*(const Scalar& k, const RistrettoPoint& p) { return p * k; }   // ristretto.rs:346-360

// ---- batch API (what a caller with many elements should use) -------------------------------
inline std::vector<EdwardsPoint> mul_batch(const std::vector<EdwardsPoint>& ps, const std::vector<Scalar>& ks)
{
    if (ps.size() != ks.size()) throw std::invalid_argument("mul_batch: size mismatch");
    if (ps.empty()) return {};                                              // (data() of an empty vector is null, which the library refuses)
    std::vector<uint64_t> p(ps.size() * 20), k(ks.size() * 5), o(ps.size() * 20);
    for (size_t i = 0; i < ps.size(); i++) {
        ps[i].flat(&p[20 * i]);
        std::memcpy(&k[5 * i], ks[i].l.data(), 40);
    }
    Backend::check(zc_ed_scalar_mul(Backend::ctx(), p.data(), k.data(), o.data(), ps.size(), ZC_SCALAR_MUL_STRICT), "zc_ed_scalar_mul");
    std::vector<EdwardsPoint> out(ps.size());
    for (size_t i = 0; i < ps.size(); i++) out[i] = EdwardsPoint::unflat(&o[20 * i]);
    return out;
}
inline std::vector<FieldElement> mul_batch(const std::vector<FieldElement>& a, const std::vector<FieldElement>& b)
{
    if (a.size() != b.size()) throw std::invalid_argument("mul_batch: size mismatch");
    if (a.empty()) return {};
    std::vector<uint64_t> x(a.size() * 5), y(a.size() * 5), o(a.size() * 5);
    for (size_t i = 0; i < a.size(); i++) {
        std::memcpy(&x[5 * i], a[i].l.data(), 40);
        std::memcpy(&y[5 * i], b[i].l.data(), 40);
    }
    Backend::check(zc_fe_mul(Backend::ctx(), x.data(), y.data(), o.data(), a.size()), "zc_fe_mul");
    std::vector<FieldElement> out(a.size());
    for (size_t i = 0; i < a.size(); i++) std::memcpy(out[i].l.data(), &o[5 * i], 40);
    return out;
}
inline std::vector<std::optional<CompressedRistretto>> ristretto_roundtrip_mul_batch(
    const std::vector<CompressedRistretto>& enc, const std::vector<Scalar>& ks)
{
    if (enc.size() != ks.size()) throw std::invalid_argument("size mismatch");
    if (enc.empty()) return {};
    std::vector<uint8_t> in(enc.size() * 32), out(enc.size() * 32), ok(enc.size());
    std::vector<uint64_t> k(ks.size() * 5);
    for (size_t i = 0; i < enc.size(); i++) {
        std::memcpy(&in[32 * i], enc[i].bytes.data(), 32);
        std::memcpy(&k[5 * i], ks[i].l.data(), 40);
    }
    Backend::check(zc_ris_roundtrip_mul(Backend::ctx(), in.data(), k.data(), out.data(), ok.data(), enc.size()), "zc_ris_roundtrip_mul");
    std::vector<std::optional<CompressedRistretto>> r(enc.size());
    for (size_t i = 0; i < enc.size(); i++)
        if (ok[i]) {
            CompressedRistretto c;
            std::memcpy(c.bytes.data(), &out[32 * i], 32);
            r[i] = c;
        }
    return r;
}

// sum_i k_i * P_i (bucket method on the GPU); equal to the fold of operator* and operator+ under ==
inline EdwardsPoint msm(const std::vector<EdwardsPoint>& ps, const std::vector<Scalar>& ks)
{
    if (ps.size() != ks.size()) throw std::invalid_argument("msm: size mismatch");
    std::vector<uint64_t> p(ps.size() * 20 + 1), k(ks.size() * 5 + 1);      // (one spare element: data() is never null, and n == 0 is the empty sum)
    for (size_t i = 0; i < ps.size(); i++) {
        ps[i].flat(&p[20 * i]);
        std::memcpy(&k[5 * i], ks[i].l.data(), 40);
    }
    uint64_t o[20];
    Backend::check(zc_msm(Backend::ctx(), p.data(), k.data(), ps.size(), o), "zc_msm");
    return EdwardsPoint::unflat(o);
}
// the exchange step of a sharded MSM: ((p_0 + p_1) + p_2) + ... in index order, one kernel launch
inline EdwardsPoint fold_ordered(const std::vector<EdwardsPoint>& ps)
{
    std::vector<uint64_t> p(ps.size() * 20 + 1);                            // (one spare element: an empty list is the library's to refuse)
    for (size_t i = 0; i < ps.size(); i++) ps[i].flat(&p[20 * i]);
    uint64_t o[20];
    Backend::check(zc_ed_fold_ordered(Backend::ctx(), p.data(), ps.size(), o), "zc_ed_fold_ordered");
    return EdwardsPoint::unflat(o);
}
// this rank's shard of a global MSM (after Backend::comm_init): all-gather of partial sums + ordered fold
inline EdwardsPoint msm_sharded(const std::vector<EdwardsPoint>& ps, const std::vector<Scalar>& ks)
{
    std::vector<uint64_t> p(ps.size() * 20), k(ks.size() * 5);
    for (size_t i = 0; i < ps.size(); i++) {
        ps[i].flat(&p[20 * i]);
        std::memcpy(&k[5 * i], ks[i].l.data(), 40);
    }
    uint64_t o[20];
    Backend::check(zc_msm_sharded(Backend::ctx(), p.data(), k.data(), ps.size(), o), "zc_msm_sharded");
    return EdwardsPoint::unflat(o);
}
// this device's partial sum left in device memory (out_dev: 160 bytes of HIP memory)
inline void msm_partial(const uint64_t* points, const uint64_t* scalars, size_t n, uint64_t* out_dev)
{
    Backend::check(zc_msm_partial(Backend::ctx(), points, scalars, n, out_dev), "zc_msm_partial");
}
// the encodings of 2 * P_i without a square root: the rows share inversions (zerocaf_hip_ext.h).  compress(k * P) for a point of
// order L is this call on (k * 2^-1 mod L) * P; a point of E[8] gives 32 zero bytes, as the reference's composition does
inline std::vector<CompressedRistretto> double_and_compress_batch(const std::vector<RistrettoPoint>& ps)
{
    std::vector<uint64_t> p(ps.size() * 20);
    std::vector<uint8_t> o(ps.size() * 32);
    for (size_t i = 0; i < ps.size(); i++) ps[i].p.flat(&p[20 * i]);
    if (!ps.empty()) Backend::check(zc_ris_double_and_compress(Backend::ctx(), p.data(), o.data(), ps.size()), "zc_ris_double_and_compress");
    std::vector<CompressedRistretto> out(ps.size());
    for (size_t i = 0; i < ps.size(); i++) std::memcpy(out[i].bytes.data(), &o[32 * i], 32);
    return out;
}
// k * BASEPOINT from the fixed-base table: equal to `BASEPOINT * k` under == (not limb-identical)
inline std::vector<EdwardsPoint> mul_base_batch(const std::vector<Scalar>& ks)
{
    if (ks.empty()) return {};                                              // (data() of an empty vector is null, which the library refuses)
    std::vector<uint64_t> k(ks.size() * 5), o(ks.size() * 20);
    for (size_t i = 0; i < ks.size(); i++) std::memcpy(&k[5 * i], ks[i].l.data(), 40);
    Backend::check(zc_ed_mul_base(Backend::ctx(), k.data(), o.data(), ks.size()), "zc_ed_mul_base");
    std::vector<EdwardsPoint> out(ks.size());
    for (size_t i = 0; i < ks.size(); i++) out[i] = EdwardsPoint::unflat(&o[20 * i]);
    return out;
}
// window_naf_mul (src/edwards.rs:155-171) with its table indexed correctly, one launch; width 2..7
inline std::vector<EdwardsPoint> window_naf_mul_batch(const std::vector<Scalar>& ks, unsigned width)
{
    if (ks.empty()) return {};
    std::vector<uint64_t> k(ks.size() * 5), o(ks.size() * 20);
    for (size_t i = 0; i < ks.size(); i++) std::memcpy(&k[5 * i], ks[i].l.data(), 40);
    Backend::check(zc_ed_mul_base_wnaf(Backend::ctx(), k.data(), width, o.data(), ks.size()), "zc_ed_mul_base_wnaf");
    std::vector<EdwardsPoint> out(ks.size());
    for (size_t i = 0; i < ks.size(); i++) out[i] = EdwardsPoint::unflat(&o[20 * i]);
    return out;
}
// the bucket method's plan for a shard of n pairs: {c, W, affine, record payload bytes, run, segment, sort passes, window groups,
// record stride, windows per group [4], run length per group [4]}
inline std::array<int32_t, 17> msm_plan(size_t n, bool points_aligned16 = true)
{
    std::array<int32_t, 17> v{};
    Backend::check(zc_msm_plan(Backend::ctx(), n, points_aligned16 ? 1 : 0, v.data(), 17), "zc_msm_plan");
    return v;
}
// `batch` independent MSMs, each over its own points (zc_msm_batch): pss[b] and kss[b] of one length n for every instance
// (pad ragged instances with zero scalars); result b equals msm(pss[b], kss[b]) under ==
inline std::vector<EdwardsPoint> msm_batch(const std::vector<std::vector<EdwardsPoint>>& pss, const std::vector<std::vector<Scalar>>& kss)
{
    if (pss.size() != kss.size()) throw std::invalid_argument("msm_batch: size mismatch");
    const size_t batch = pss.size(), n = batch ? pss[0].size() : 0;
    std::vector<uint64_t> p(batch * n * 20 + 1), k(batch * n * 5 + 1), o(batch * 20);      // (one spare element: instances of no pairs are identities)
    for (size_t b = 0; b < batch; b++) {
        if (pss[b].size() != n || kss[b].size() != n) throw std::invalid_argument("msm_batch: instances of different lengths");
        for (size_t i = 0; i < n; i++) {
            pss[b][i].flat(&p[20 * (b * n + i)]);
            std::memcpy(&k[5 * (b * n + i)], kss[b][i].l.data(), 40);
        }
    }
    Backend::check(zc_msm_batch(Backend::ctx(), p.data(), k.data(), n, batch, o.data()), "zc_msm_batch");
    std::vector<EdwardsPoint> out(batch);
    for (size_t b = 0; b < batch; b++) out[b] = EdwardsPoint::unflat(&o[20 * b]);
    return out;
}
// Short linear combinations, one per row (zc_ed_lincomb): out[i] = sum_j kss[i][j] * pss[i][j], 1..8 terms of one count for
// every row (pad ragged rows with zero scalars); row i equals ((k0*P0 + k1*P1) + ...) under ==.  One doubling chain per row
// is shared by its terms: for 2..8 terms per row this is the call, from 64 pairs per instance on msm_batch.
inline std::vector<EdwardsPoint> ed_lincomb(const std::vector<std::vector<EdwardsPoint>>& pss, const std::vector<std::vector<Scalar>>& kss)
{
    if (pss.size() != kss.size()) throw std::invalid_argument("ed_lincomb: size mismatch");
    const size_t n = pss.size(), t = n ? pss[0].size() : 1;
    std::vector<uint64_t> p(n * t * 20), k(n * t * 5), o(n * 20);
    for (size_t i = 0; i < n; i++) {
        if (pss[i].size() != t || kss[i].size() != t) throw std::invalid_argument("ed_lincomb: rows of different lengths");
        for (size_t j = 0; j < t; j++) {
            pss[i][j].flat(&p[20 * (i * t + j)]);
            std::memcpy(&k[5 * (i * t + j)], kss[i][j].l.data(), 40);
        }
    }
    if (n == 0) return {};
    Backend::check(zc_ed_lincomb(Backend::ctx(), p.data(), k.data(), t, o.data(), n), "zc_ed_lincomb");
    std::vector<EdwardsPoint> out(n);
    for (size_t i = 0; i < n; i++) out[i] = EdwardsPoint::unflat(&o[20 * i]);
    return out;
}
// Wire-format linear combinations, one per row (zc_ris_lincomb): compress(bs[i] * RISTRETTO_BASEPOINT + sum_j kss[i][j] *
// decompress(ess[i][j])), bit-identical to the reference's composition; 1..8 terms of one count for every row, 1..7 with a
// base term (bs empty: none).  first: the encodings (32 zero bytes where a term did not decode), second: the accept mask.
inline std::pair<std::vector<CompressedRistretto>, std::vector<uint8_t>> ris_lincomb(const std::vector<std::vector<CompressedRistretto>>& ess,
                                                                                     const std::vector<std::vector<Scalar>>& kss,
                                                                                     const std::vector<Scalar>& bs = {})
{
    if (ess.size() != kss.size() || (!bs.empty() && bs.size() != ess.size())) throw std::invalid_argument("ris_lincomb: size mismatch");
    const size_t n = ess.size(), t = n ? ess[0].size() : 1;
    std::vector<uint8_t> e(n * t * 32), o(n * 32), ok(n);
    std::vector<uint64_t> k(n * t * 5), b(bs.size() * 5);
    for (size_t i = 0; i < n; i++) {
        if (ess[i].size() != t || kss[i].size() != t) throw std::invalid_argument("ris_lincomb: rows of different lengths");
        for (size_t j = 0; j < t; j++) {
            std::memcpy(&e[32 * (i * t + j)], ess[i][j].bytes.data(), 32);
            std::memcpy(&k[5 * (i * t + j)], kss[i][j].l.data(), 40);
        }
        if (!bs.empty()) std::memcpy(&b[5 * i], bs[i].l.data(), 40);
    }
    std::vector<CompressedRistretto> out(n);
    if (n == 0) return {out, ok};
    Backend::check(zc_ris_lincomb(Backend::ctx(), e.data(), k.data(), t, bs.empty() ? nullptr : b.data(), o.data(), ok.data(), n), "zc_ris_lincomb");
    for (size_t i = 0; i < n; i++) std::memcpy(out[i].bytes.data(), &o[32 * i], 32);
    return {out, ok};
}
// The weighted sum of all rows as one MSM (zc_ris_lincomb_sum, zerocaf_hip_ext_sum.h through zerocaf_hip_ext.h): compress(b * RISTRETTO_BASEPOINT + sum_i
// sum_j w_ij * decompress(ess[i][j])) with w_ij = zs[i] * kss[i][j] mod L and b = sum_i zs[i] * bs[i] mod L, every scalar read
// by value (bs empty: no base term; zs empty: no weights).  A row with an undecodable term has mask 0 and is left out of both
// sums.  first: the encoding of the sum, second: the accept mask.  A batch verifies when the mask is all ones and the bytes zero.
inline std::pair<CompressedRistretto, std::vector<uint8_t>> ris_lincomb_sum(const std::vector<std::vector<CompressedRistretto>>& ess,
                                                                            const std::vector<std::vector<Scalar>>& kss,
                                                                            const std::vector<Scalar>& bs = {}, const std::vector<Scalar>& zs = {})
{
    if (ess.size() != kss.size() || (!bs.empty() && bs.size() != ess.size()) || (!zs.empty() && zs.size() != ess.size()))
        throw std::invalid_argument("ris_lincomb_sum: size mismatch");
    const size_t n = ess.size(), t = n ? ess[0].size() : 1;
    std::vector<uint8_t> e(n * t * 32 + 1), ok(n);                  // (one spare element: data() is never null, and n == 0 is the empty sum)
    std::vector<uint64_t> k(n * t * 5 + 1), b(bs.size() * 5), z(zs.size() * 5);
    for (size_t i = 0; i < n; i++) {
        if (ess[i].size() != t || kss[i].size() != t) throw std::invalid_argument("ris_lincomb_sum: rows of different lengths");
        for (size_t j = 0; j < t; j++) {
            std::memcpy(&e[32 * (i * t + j)], ess[i][j].bytes.data(), 32);
            std::memcpy(&k[5 * (i * t + j)], kss[i][j].l.data(), 40);
        }
        if (!bs.empty()) std::memcpy(&b[5 * i], bs[i].l.data(), 40);
        if (!zs.empty()) std::memcpy(&z[5 * i], zs[i].l.data(), 40);
    }
    CompressedRistretto out;
    uint8_t o[32];
    Backend::check(zc_ris_lincomb_sum(Backend::ctx(), e.data(), k.data(), t, bs.empty() ? nullptr : b.data(), zs.empty() ? nullptr : z.data(), o, ok.data(), n),
                   "zc_ris_lincomb_sum");
    std::memcpy(out.bytes.data(), o, 32);
    return {out, ok};
}
// ONE scalar for a whole batch (zc_ed_scalar_mul_shared / zc_ris_mul_shared, zerocaf_hip_ext_shared.h through zerocaf_hip_ext.h): a view
// key against every output, an OPRF key against every client point.  The scalar is recoded once on the host; the running time
// depends on it.  ps[i] * k under == (identical encodings, another projective representative than the reference's).
inline std::vector<EdwardsPoint> scalar_mul_shared(const std::vector<EdwardsPoint>& ps, const Scalar& k)
{
    std::vector<uint64_t> p(ps.size() * 20), o(ps.size() * 20);
    for (size_t i = 0; i < ps.size(); i++) ps[i].flat(&p[20 * i]);
    if (!ps.empty()) Backend::check(zc_ed_scalar_mul_shared(Backend::ctx(), p.data(), k.l.data(), o.data(), ps.size()), "zc_ed_scalar_mul_shared");
    std::vector<EdwardsPoint> out(ps.size());
    for (size_t i = 0; i < ps.size(); i++) out[i] = EdwardsPoint::unflat(&o[20 * i]);
    return out;
}
// compress(k * decompress(es[i])), byte-identical to the reference's composition.  first: the encodings (32 zero bytes where a
// row did not decode, or where the product is the identity), second: the accept mask.
inline std::pair<std::vector<CompressedRistretto>, std::vector<uint8_t>> ris_mul_shared(const std::vector<CompressedRistretto>& es, const Scalar& k)
{
    const size_t n = es.size();
    std::vector<uint8_t> e(n * 32), o(n * 32), ok(n);
    for (size_t i = 0; i < n; i++) std::memcpy(&e[32 * i], es[i].bytes.data(), 32);
    std::vector<CompressedRistretto> out(n);
    if (n == 0) return {out, ok};
    Backend::check(zc_ris_mul_shared(Backend::ctx(), e.data(), k.l.data(), o.data(), ok.data(), n), "zc_ris_mul_shared");
    for (size_t i = 0; i < n; i++) std::memcpy(out[i].bytes.data(), &o[32 * i], 32);
    return {out, ok};
}
// ONE scalar VECTOR for a whole batch (zc_ed_lincomb_shared / zc_ris_lincomb_shared, zerocaf_hip_ext_shared_lincomb.h through
// zerocaf_hip_ext.h): out[i] = sum_j ks[j] * pss[i][j] with the same 1..8 coefficients in every row -- ElGamal decryption under one
// key (1, -x), threshold share combination (the Lagrange coefficients), generator folding (u^-1, u).  The terms' recodings are merged
// into one schedule on the host; the running time depends on ks.  Row i equals ((k0*P0 + k1*P1) + ...) under ==.
inline std::vector<EdwardsPoint> ed_lincomb_shared(const std::vector<std::vector<EdwardsPoint>>& pss, const std::vector<Scalar>& ks)
{
    const size_t n = pss.size(), t = ks.size();
    std::vector<uint64_t> p(n * t * 20), k(t * 5), o(n * 20);
    for (size_t j = 0; j < t; j++) std::memcpy(&k[5 * j], ks[j].l.data(), 40);
    for (size_t i = 0; i < n; i++) {
        if (pss[i].size() != t) throw std::invalid_argument("ed_lincomb_shared: a row without one point per scalar");
        for (size_t j = 0; j < t; j++) pss[i][j].flat(&p[20 * (i * t + j)]);
    }
    if (n) Backend::check(zc_ed_lincomb_shared(Backend::ctx(), p.data(), k.data(), t, o.data(), n), "zc_ed_lincomb_shared");
    std::vector<EdwardsPoint> out(n);
    for (size_t i = 0; i < n; i++) out[i] = EdwardsPoint::unflat(&o[20 * i]);
    return out;
}
// compress(sum_j ks[j] * decompress(ess[i][j])), byte-identical to ris_lincomb without a base term and with ks in every row.
// first: the encodings (32 zero bytes where a term did not decode, or where the sum is the identity), second: the accept mask.
// No basepoint term: pass the encoding of B as a term.
inline std::pair<std::vector<CompressedRistretto>, std::vector<uint8_t>> ris_lincomb_shared(const std::vector<std::vector<CompressedRistretto>>& ess,
                                                                                            const std::vector<Scalar>& ks)
{
    const size_t n = ess.size(), t = ks.size();
    std::vector<uint8_t> e(n * t * 32), o(n * 32), ok(n);
    std::vector<uint64_t> k(t * 5);
    for (size_t j = 0; j < t; j++) std::memcpy(&k[5 * j], ks[j].l.data(), 40);
    for (size_t i = 0; i < n; i++) {
        if (ess[i].size() != t) throw std::invalid_argument("ris_lincomb_shared: a row without one encoding per scalar");
        for (size_t j = 0; j < t; j++) std::memcpy(&e[32 * (i * t + j)], ess[i][j].bytes.data(), 32);
    }
    std::vector<CompressedRistretto> out(n);
    if (n == 0) return {out, ok};
    Backend::check(zc_ris_lincomb_shared(Backend::ctx(), e.data(), k.data(), t, o.data(), ok.data(), n), "zc_ris_lincomb_shared");
    for (size_t i = 0; i < n; i++) std::memcpy(out[i].bytes.data(), &o[32 * i], 32);
    return {out, ok};
}
// SHA-512 over batched rows (zc_sha512_rows / zc_sc_from_sha512 / zc_ris_from_sha512, zerocaf_hip_ext_hash.h through
// zerocaf_hip_ext.h): the message of row i is prefix || parts[0][i] || parts[1][i] || ..., parts[j] = n rows of part_len[j]
// contiguous bytes (1..4 parts, a prefix of at most 256 bytes, rows of at most 65535).  Host or device pointers, all of one kind.
struct HashParts {
    std::vector<const uint8_t*> ptr;
    std::vector<size_t> len;
    void add(const uint8_t* rows, size_t row_bytes)
    {
        ptr.push_back(rows);
        len.push_back(row_bytes);
    }
};
// out64: n x 64 bytes, the digests in FIPS 180-4 byte order
inline void sha512_rows(const std::string& prefix, const HashParts& parts, uint8_t* out64, size_t n)
{
    Backend::check(zc_sha512_rows(Backend::ctx(), reinterpret_cast<const uint8_t*>(prefix.data()), prefix.size(), parts.ptr.data(), parts.len.data(), parts.ptr.size(), out64, n),
                   "zc_sha512_rows");
}
// out: n x 5 limbs, the digest as a little-endian 512-bit integer mod L (zc_sc_from_bytes_wide without the digest in memory)
inline void sc_from_sha512(const std::string& prefix, const HashParts& parts, uint64_t* out, size_t n)
{
    Backend::check(zc_sc_from_sha512(Backend::ctx(), reinterpret_cast<const uint8_t*>(prefix.data()), prefix.size(), parts.ptr.data(), parts.len.data(), parts.ptr.size(), out, n),
                   "zc_sc_from_sha512");
}
// out: n x 20 limbs, from_uniform_bytes of the digest (zc_ris_from_uniform_bytes likewise)
inline void ris_from_sha512(const std::string& prefix, const HashParts& parts, uint64_t* out, size_t n)
{
    Backend::check(zc_ris_from_sha512(Backend::ctx(), reinterpret_cast<const uint8_t*>(prefix.data()), prefix.size(), parts.ptr.data(), parts.len.data(), parts.ptr.size(), out, n),
                   "zc_ris_from_sha512");
}
// {regime (0 = scalar multiplications + folds, 1 = buckets), c, W, affine, run length, segment buckets, sort passes, record
// stride bytes} of a batch of `batch` instances of n pairs
inline std::array<int32_t, 8> msm_batch_plan(size_t n, size_t batch, bool points_aligned16 = true)
{
    std::array<int32_t, 8> v{};
    Backend::check(zc_msm_batch_plan(Backend::ctx(), n, batch, points_aligned16 ? 1 : 0, v.data(), 8), "zc_msm_batch_plan");
    return v;
}
// A fixed-base MSM table (zc_msm_bases_create), freed when the object goes: msm() of one or many scalar vectors against the
// same bases, each result equal to msm(bases, ks) under ==
class MsmBases {
public:
    explicit MsmBases(const std::vector<EdwardsPoint>& ps, int window_bits = 0) : n_(ps.size())
    {
        std::vector<uint64_t> p(ps.size() * 20);
        for (size_t i = 0; i < ps.size(); i++) ps[i].flat(&p[20 * i]);
        Backend::check(zc_msm_bases_create(Backend::ctx(), p.data(), ps.size(), window_bits, &id_), "zc_msm_bases_create");
    }
    MsmBases(const MsmBases&) = delete;
    MsmBases& operator=(const MsmBases&) = delete;
    MsmBases(MsmBases&& o) noexcept : id_(o.id_), n_(o.n_) { o.id_ = 0; }
    MsmBases& operator=(MsmBases&& o) noexcept
    {
        if (this != &o) {
            reset();
            id_ = o.id_;
            n_ = o.n_;
            o.id_ = 0;
        }
        return *this;
    }
    ~MsmBases() { reset(); }
    size_t size() const { return n_; }
    // kss: batch vectors of size() scalars each -> batch sums
    std::vector<EdwardsPoint> msm(const std::vector<std::vector<Scalar>>& kss) const
    {
        std::vector<uint64_t> k(kss.size() * n_ * 5), o(kss.size() * 20);
        for (size_t b = 0; b < kss.size(); b++) {
            if (kss[b].size() != n_) throw std::invalid_argument("MsmBases::msm: a scalar vector of the wrong length");
            for (size_t i = 0; i < n_; i++) std::memcpy(&k[5 * (b * n_ + i)], kss[b][i].l.data(), 40);
        }
        Backend::check(zc_msm_fixed(Backend::ctx(), id_, k.data(), kss.size(), o.data()), "zc_msm_fixed");
        std::vector<EdwardsPoint> out(kss.size());
        for (size_t b = 0; b < kss.size(); b++) out[b] = EdwardsPoint::unflat(&o[20 * b]);
        return out;
    }
    EdwardsPoint msm(const std::vector<Scalar>& ks) const { return msm(std::vector<std::vector<Scalar>>{ks})[0]; }
    // {c, W, record stride bytes, run length, segment buckets, sort passes, table MiB, window groups} of a table of n bases
    static std::array<int32_t, 8> plan(size_t n, int window_bits = 0)
    {
        std::array<int32_t, 8> v{};
        Backend::check(zc_msm_fixed_plan(Backend::ctx(), n, window_bits, v.data(), 8), "zc_msm_fixed_plan");
        return v;
    }

private:
    void reset()
    {
        if (id_) zc_msm_bases_destroy(Backend::ctx(), id_);
        id_ = 0;
    }
    uint64_t id_ = 0;
    size_t n_ = 0;
};
// key generation: (RISTRETTO_BASEPOINT * k).compress(), identical bytes
inline std::vector<CompressedRistretto> ristretto_keygen_batch(const std::vector<Scalar>& ks)
{
    if (ks.empty()) return {};
    std::vector<uint64_t> k(ks.size() * 5);
    std::vector<uint8_t> o(ks.size() * 32);
    for (size_t i = 0; i < ks.size(); i++) std::memcpy(&k[5 * i], ks[i].l.data(), 40);
    Backend::check(zc_ris_mul_base_compress(Backend::ctx(), k.data(), o.data(), ks.size()), "zc_ris_mul_base_compress");
    std::vector<CompressedRistretto> out(ks.size());
    for (size_t i = 0; i < ks.size(); i++) std::memcpy(out[i].bytes.data(), &o[32 * i], 32);
    return out;
}
// A generator set (zc_gens_create, zerocaf_hip_ext_gens.h through zerocaf_hip_ext.h), freed when the object goes: 1..8 fixed points
// of the caller's with a comb table each -- the second Pedersen generator, a recipient key, the bases of a DLEQ proof.  mul() and
// mul_compress() are mul_base_batch and ristretto_keygen_batch over them: row i is ((kss[i][0]*G_0 + kss[i][1]*G_1) + ...) under ==.
// A point that is not on the curve is refused (std::runtime_error from Backend::check).  Nothing is constant-time.
class Generators {
public:
    explicit Generators(const std::vector<EdwardsPoint>& gs) : count_(gs.size())
    {
        std::vector<uint64_t> p(gs.size() * 20);
        for (size_t j = 0; j < gs.size(); j++) gs[j].flat(&p[20 * j]);
        Backend::check(zc_gens_create(Backend::ctx(), p.data(), gs.size(), &id_), "zc_gens_create");
    }
    Generators(const Generators&) = delete;
    Generators& operator=(const Generators&) = delete;
    Generators(Generators&& o) noexcept : id_(o.id_), count_(o.count_) { o.id_ = 0; }
    Generators& operator=(Generators&& o) noexcept
    {
        if (this != &o) {
            reset();
            id_ = o.id_;
            count_ = o.count_;
            o.id_ = 0;
        }
        return *this;
    }
    ~Generators() { reset(); }
    size_t size() const { return count_; }
    std::vector<EdwardsPoint> mul(const std::vector<std::vector<Scalar>>& kss) const
    {
        std::vector<uint64_t> k = flat(kss), o(kss.size() * 20);
        if (!kss.empty()) Backend::check(zc_ed_mul_gens(Backend::ctx(), id_, k.data(), o.data(), kss.size()), "zc_ed_mul_gens");
        std::vector<EdwardsPoint> out(kss.size());
        for (size_t i = 0; i < kss.size(); i++) out[i] = EdwardsPoint::unflat(&o[20 * i]);
        return out;
    }
    std::vector<CompressedRistretto> mul_compress(const std::vector<std::vector<Scalar>>& kss) const
    {
        std::vector<uint64_t> k = flat(kss);
        std::vector<uint8_t> o(kss.size() * 32);
        if (!kss.empty()) Backend::check(zc_ris_mul_gens_compress(Backend::ctx(), id_, k.data(), o.data(), kss.size()), "zc_ris_mul_gens_compress");
        std::vector<CompressedRistretto> out(kss.size());
        for (size_t i = 0; i < kss.size(); i++) std::memcpy(out[i].bytes.data(), &o[32 * i], 32);
        return out;
    }

private:
    void reset()
    {
        if (id_) zc_gens_destroy(Backend::ctx(), id_);
        id_ = 0;
    }
    std::vector<uint64_t> flat(const std::vector<std::vector<Scalar>>& kss) const
    {
        std::vector<uint64_t> k(kss.size() * count_ * 5);
        for (size_t i = 0; i < kss.size(); i++) {
            if (kss[i].size() != count_) throw std::invalid_argument("Generators: a row without one scalar per generator");
            for (size_t j = 0; j < count_; j++) std::memcpy(&k[5 * (i * count_ + j)], kss[i][j].l.data(), 40);
        }
        return k;
    }
    uint64_t id_ = 0;
    size_t count_ = 0;
};
// Point sums (zc_ed_sum_rows / zc_ris_sum_rows, zerocaf_hip_ext_sum_rows.h through zerocaf_hip_ext.h): row i is rows[i][0] + rows[i][1] + ...
// under the unified addition, associated in the order the header fixes for the row length (a left fold up to 32 terms, strided
// slices and a pairwise tree above) -- an ElGamal tally, an aggregate of keys or commitments.  Every row has the same length
// (pad with EdwardsPoint::identity() / the zero encoding); empty rows give the identity.
inline std::vector<EdwardsPoint> sum_rows(const std::vector<std::vector<EdwardsPoint>>& rows)
{
    const size_t n = rows.size(), terms = n ? rows[0].size() : 0;
    std::vector<uint64_t> p(n * terms * 20 + 20), o(n * 20);
    for (size_t i = 0; i < n; i++) {
        if (rows[i].size() != terms) throw std::invalid_argument("sum_rows: rows of different lengths");
        for (size_t j = 0; j < terms; j++) rows[i][j].flat(&p[20 * (i * terms + j)]);
    }
    if (n) Backend::check(zc_ed_sum_rows(Backend::ctx(), p.data(), terms, o.data(), n), "zc_ed_sum_rows");
    std::vector<EdwardsPoint> out(n);
    for (size_t i = 0; i < n; i++) out[i] = EdwardsPoint::unflat(&o[20 * i]);
    return out;
}
// The same between the Ristretto codecs: compress(sum_j decompress(rows[i][j])); ok[i] = 0 (and 32 zero bytes) where a term does not decode.
inline std::vector<CompressedRistretto> sum_rows(const std::vector<std::vector<CompressedRistretto>>& rows, std::vector<uint8_t>* ok = nullptr)
{
    const size_t n = rows.size(), terms = n ? rows[0].size() : 0;
    std::vector<uint8_t> in(n * terms * 32 + 32), o(n * 32), accept(n);
    for (size_t i = 0; i < n; i++) {
        if (rows[i].size() != terms) throw std::invalid_argument("sum_rows: rows of different lengths");
        for (size_t j = 0; j < terms; j++) std::memcpy(&in[32 * (i * terms + j)], rows[i][j].bytes.data(), 32);
    }
    if (n) Backend::check(zc_ris_sum_rows(Backend::ctx(), in.data(), terms, o.data(), accept.data(), n), "zc_ris_sum_rows");
    std::vector<CompressedRistretto> out(n);
    for (size_t i = 0; i < n; i++) std::memcpy(out[i].bytes.data(), &o[32 * i], 32);
    if (ok) *ok = accept;
    return out;
}

namespace constants {
// src/backend/u64/constants.rs:188-211
inline EdwardsPoint BASEPOINT()
{
    return {FieldElement(std::array<uint64_t, 5>{276718085098056ull, 1646536057461434ull, 2704687245600312ull, 2630386667454967ull, 13476148227069ull}),
            FieldElement(std::array<uint64_t, 5>{1303868825475266ull, 3250718520537114ull, 2702159777242978ull, 2702159776422297ull, 10555311626649ull}),
            FieldElement::one(),
            FieldElement(std::array<uint64_t, 5>{3634527586288175ull, 2006028620404053ull, 3424252198034825ull, 2478951925947079ull, 4567251727358ull})};
}
inline RistrettoPoint RISTRETTO_BASEPOINT() { return {BASEPOINT()}; }
inline Scalar L() { return Scalar(std::array<uint64_t, 5>{1129677152307299ull, 1363544697812651ull, 714439ull, 0, 2199023255552ull}); }   // :8-9
inline FieldElement EDWARDS_D() { return FieldElement(std::array<uint64_t, 5>{3304133203739795ull, 2446467598308289ull, 1534112949566882ull, 2032729967918914ull, 2313225441931ull}); }  // :86-92
}  // namespace constants

}  // namespace zerocaf
