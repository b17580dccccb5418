// Driver of the CPU tier of the C++ mirror's tests (tests/test_cpp_mirror_calls.py): calls every function of zerocaf.hpp that
// reaches a zc_ symbol, linked against the recording stand-in (tests/cpp/mirror_standin.py), with inputs the Python test can
// rebuild from a formula, and prints what every wrapper returned.  Needs no GPU.
//
// Inputs: limb w of element (array a, row i, term j) is (a << 40) | (i << 24) | (j << 8) | w; a point is 20 such limbs
// (X 0..4, Y 5..9, Z 10..14, T 15..19); byte b of a byte element is a, i, j for b = 0, 1, 2 and (13 b + a + i + j) & 255 behind.
// Output: one segment per wrapper call.  "@ <wrapper> <key>=<value> ..." is written to stdout AND appended to the stand-in's log
// (ZC_STANDIN_LOG), so that the records of a segment are the lines between two marks; then "= <name> <hex bytes>" per returned
// object, or "! <exception type> <what>" where the wrapper threw.
#include <cstdio>
#include <cstdlib>
#include <string>
#include "zerocaf.hpp"

using namespace zerocaf;
typedef std::vector<std::vector<EdwardsPoint>> PtRows;
typedef std::vector<std::vector<Scalar>> ScRows;
typedef std::vector<std::vector<CompressedRistretto>> EncRows;

static uint64_t limb(int a, size_t i, size_t j, int w) { return ((uint64_t)a << 40) | ((uint64_t)i << 24) | ((uint64_t)j << 8) | (uint64_t)w; }
static uint8_t byte_of(int a, size_t i, size_t j, size_t b) { return (uint8_t)(b == 0 ? a : b == 1 ? i : b == 2 ? j : (13 * b + a + i + j) & 255); }
static FieldElement fe_at(int a, size_t i, size_t j, int w0)
{
    FieldElement f;
    for (int w = 0; w < 5; w++) f.l[w] = limb(a, i, j, w0 + w);
    return f;
}
static FieldElement F(int a, size_t i = 0, size_t j = 0) { return fe_at(a, i, j, 0); }
static Scalar S(int a, size_t i = 0, size_t j = 0) { return Scalar(fe_at(a, i, j, 0).l); }
static EdwardsPoint P(int a, size_t i = 0, size_t j = 0) { return {fe_at(a, i, j, 0), fe_at(a, i, j, 5), fe_at(a, i, j, 10), fe_at(a, i, j, 15)}; }
static ProjectivePoint PJ(int a) { return {fe_at(a, 0, 0, 0), fe_at(a, 0, 0, 5), fe_at(a, 0, 0, 10)}; }
template <size_t N>
static std::array<uint8_t, N> B(int a, size_t i = 0, size_t j = 0)
{
    std::array<uint8_t, N> r{};
    for (size_t b = 0; b < N; b++) r[b] = byte_of(a, i, j, b);
    return r;
}
static CompressedRistretto E(int a, size_t i = 0, size_t j = 0) { CompressedRistretto c; c.bytes = B<32>(a, i, j); return c; }
static std::vector<Scalar> scalars(int a, size_t n) { std::vector<Scalar> v; for (size_t i = 0; i < n; i++) v.push_back(S(a, i)); return v; }
static std::vector<EdwardsPoint> points(int a, size_t n) { std::vector<EdwardsPoint> v; for (size_t i = 0; i < n; i++) v.push_back(P(a, i)); return v; }
static std::vector<CompressedRistretto> encs(int a, size_t n) { std::vector<CompressedRistretto> v; for (size_t i = 0; i < n; i++) v.push_back(E(a, i)); return v; }
static ScRows sc_rows(int a, size_t n, size_t t) { ScRows v(n); for (size_t i = 0; i < n; i++) for (size_t j = 0; j < t; j++) v[i].push_back(S(a, i, j)); return v; }
static PtRows pt_rows(int a, size_t n, size_t t) { PtRows v(n); for (size_t i = 0; i < n; i++) for (size_t j = 0; j < t; j++) v[i].push_back(P(a, i, j)); return v; }
static EncRows enc_rows(int a, size_t n, size_t t) { EncRows v(n); for (size_t i = 0; i < n; i++) for (size_t j = 0; j < t; j++) v[i].push_back(E(a, i, j)); return v; }

// ---- printing
static void hex(const void* p, size_t bytes) { for (size_t i = 0; i < bytes; i++) std::printf("%02x", static_cast<const unsigned char*>(p)[i]); }
static void put_bytes(const char* name, const void* p, size_t bytes) { std::printf("= %s ", name); hex(p, bytes); std::printf("\n"); }
static void put(const char* name, const FieldElement& f) { put_bytes(name, f.l.data(), 40); }
static void put(const char* name, const Scalar& f) { put_bytes(name, f.l.data(), 40); }
static void put(const char* name, bool b) { std::printf("= %s %s\n", name, b ? "01" : "00"); }
static void put(const char* name, const std::string& s) { std::printf("= %s ", name); hex(s.data(), s.size()); std::printf("\n"); }
static void put_int(const char* name, long long v) { std::printf("= %s %lld\n", name, v); }
static void put(const char* name, const EdwardsPoint& p) { uint64_t o[20]; p.flat(o); put_bytes(name, o, 160); }
static void put(const char* name, const ProjectivePoint& p) { uint64_t o[15]; p.flat(o); put_bytes(name, o, 120); }
static void put(const char* name, const CompressedRistretto& c) { put_bytes(name, c.bytes.data(), 32); }
template <class T, size_t N>
static void put(const char* name, const std::array<T, N>& a) { put_bytes(name, a.data(), N * sizeof(T)); }
static void put(const char* name, const std::vector<uint8_t>& v) { put_bytes(name, v.data(), v.size()); }
static void put(const char* name, const std::vector<EdwardsPoint>& v)
{
    std::printf("= %s ", name);
    for (const EdwardsPoint& p : v) { uint64_t o[20]; p.flat(o); hex(o, 160); }
    std::printf("\n");
}
static void put(const char* name, const std::vector<FieldElement>& v) { std::printf("= %s ", name); for (const auto& f : v) hex(f.l.data(), 40); std::printf("\n"); }
static void put(const char* name, const std::vector<CompressedRistretto>& v) { std::printf("= %s ", name); for (const auto& c : v) hex(c.bytes.data(), 32); std::printf("\n"); }

static void mark(const std::string& label)
{
    std::printf("@ %s\n", label.c_str());
    std::fflush(stdout);
    if (const char* path = std::getenv("ZC_STANDIN_LOG"))
        if (FILE* f = std::fopen(path, "a")) { std::fprintf(f, "@ %s\n", label.c_str()); std::fclose(f); }
}
// a reference to a callable for the length of one call (std::function costs seconds of g++ time over this many lambdas)
struct Body {
    const void* obj;
    void (*call)(const void*);
    template <class F>
    Body(const F& f) : obj(&f), call([](const void* p) { (*static_cast<const F*>(p))(); }) {}
    void operator()() const { call(obj); }
};
static void seg(const std::string& label, const Body& body)
{
    mark(label);
    try { body(); }
    catch (const std::invalid_argument& e) { std::printf("! invalid_argument %s\n", e.what()); }
    catch (const std::domain_error& e) { std::printf("! domain_error %s\n", e.what()); }
    catch (const std::runtime_error& e) { std::printf("! runtime_error %s\n", e.what()); }
}
static std::string kv(const char* k, size_t v) { return std::string(" ") + k + "=" + std::to_string(v); }

int main()
{
    // ---- Backend
    seg("Backend::ctx", [] { put("nonnull", Backend::ctx() != nullptr); });
    seg("Backend::check", [] { Backend::check(0, "nothing"); Backend::check(-1, "probe"); });
    seg("Backend::device_count", [] { put_int("ret", Backend::device_count()); });
    seg("Backend::version", [] { put("ret", Backend::version()); });
    seg("Backend::set_stream", [] { Backend::set_stream(reinterpret_cast<void*>(0x1230)); });
    seg("Backend::use_own_stream", [] { Backend::use_own_stream(); });
    seg("Backend::synchronize", [] { Backend::synchronize(); });
    seg("Backend::device", [] { put_int("ret", Backend::device(2)); });
    seg("Backend::slot_count", [] { put_int("ret", Backend::slot_count()); });
    seg("Backend::set_stream_dev", [] { Backend::set_stream_dev(3, reinterpret_cast<void*>(0x4560)); });
    seg("Backend::host_register", [] { Backend::host_register(reinterpret_cast<void*>(0x7890), 4096); });
    seg("Backend::host_unregister", [] { Backend::host_unregister(reinterpret_cast<void*>(0x7890)); });
    seg("Backend::comm_unique_id", [] { put("ret", Backend::comm_unique_id()); });
    seg("Backend::comm_init", [] { Backend::comm_init(B<128>(1), 2, 5); });
    seg("Backend::comm_size", [] { put_int("ret", Backend::comm_size()); });
    seg("Backend::comm_destroy", [] { Backend::comm_destroy(); });

    // ---- FieldElement
    seg("FieldElement::operator+", [] { put("ret", F(1) + F(2)); });
    seg("FieldElement::operator-", [] { put("ret", F(1) - F(2)); });
    seg("FieldElement::operator*", [] { put("ret", F(1) * F(2)); });
    seg("FieldElement::neg", [] { put("ret", -F(1)); });
    seg("FieldElement::square", [] { put("ret", F(1).square()); });
    seg("FieldElement::inverse", [] { put("ret", F(1).inverse()); });
    seg("FieldElement::operator/", [] { put("ret", F(1) / F(2)); });
    seg("FieldElement::half", [] { put("ret", F(1).half()); });
    seg("FieldElement::pow", [] { put("ret", F(1).pow(F(2))); });
    seg("FieldElement::legendre_symbol", [] { put("ret", F(1).legendre_symbol()); });
    seg("FieldElement::is_positive", [] { put("ret", F(1).is_positive()); });
    seg("FieldElement::mod_sqrt sign=1", [] { const auto r = F(1).mod_sqrt(true); put("has", r.has_value()); if (r) put("ret", *r); });
    seg("FieldElement::mod_sqrt sign=0", [] { const auto r = F(1).mod_sqrt(false); put("has", r.has_value()); if (r) put("ret", *r); });
    seg("FieldElement::sqrt_ratio_i", [] { const auto r = F(1).sqrt_ratio_i(F(2)); put("first", r.first); put("second", r.second); });
    seg("FieldElement::inv_sqrt", [] { const auto r = F(1).inv_sqrt(); put("first", r.first); put("second", r.second); });
    seg("FieldElement::from_bytes", [] { put("ret", FieldElement::from_bytes(B<32>(1))); });
    seg("FieldElement::to_bytes", [] { put("ret", F(1).to_bytes()); });
    seg("FieldElement::operator==", [] { put("ret", F(1) == F(2)); });

    // ---- Scalar
    seg("Scalar::operator+", [] { put("ret", S(1) + S(2)); });
    seg("Scalar::operator-", [] { put("ret", S(1) - S(2)); });
    seg("Scalar::operator*", [] { put("ret", S(1) * S(2)); });
    seg("Scalar::neg", [] { put("ret", -S(1)); });
    seg("Scalar::square", [] { put("ret", S(1).square()); });
    seg("Scalar::half", [] { put("ret", S(1).half()); });
    seg("Scalar::pow", [] { put("ret", S(1).pow(S(2))); });
    seg("Scalar::operator>>", [] { put("ret", S(1) >> 9); });
    seg("Scalar::into_bits", [] { put("ret", S(1).into_bits()); });
    seg("Scalar::compute_NAF", [] { put("ret", S(1).compute_NAF()); });
    seg("Scalar::compute_window_NAF", [] { put("ret", S(1).compute_window_NAF(5)); });
    seg("Scalar::from_bytes", [] { put("ret", Scalar::from_bytes(B<32>(1))); });
    seg("Scalar::from_bytes_wide", [] { put("ret", Scalar::from_bytes_wide(B<64>(1))); });
    seg("Scalar::from_bytes_mod_order", [] { put("ret", Scalar::from_bytes_mod_order(B<32>(1))); });
    seg("Scalar::muladd", [] { put("ret", S(1).muladd(S(2), S(3))); });
    seg("Scalar::invert", [] { put("ret", S(1).invert()); });
    seg("Scalar::to_bytes", [] { put("ret", S(1).to_bytes()); });
    seg("Scalar::operator==", [] { put("ret", S(1) == S(2)); });

    // ---- points
    seg("EdwardsPoint::operator+", [] { put("ret", P(1) + P(2)); });
    seg("EdwardsPoint::operator-", [] { put("ret", P(1) - P(2)); });
    seg("EdwardsPoint::neg", [] { put("ret", -P(1)); });
    seg("EdwardsPoint::double_", [] { put("ret", P(1).double_()); });
    seg("EdwardsPoint::operator*", [] { put("ret", P(1) * S(2)); });
    seg("EdwardsPoint::operator==", [] { put("ret", P(1) == P(2)); });
    seg("EdwardsPoint::is_valid", [] { put("ret", P(1).is_valid()); });
    seg("EdwardsPoint::compress", [] { put("ret", P(1).compress().bytes); });
    seg("AffinePoint::from", [] { const AffinePoint a = AffinePoint::from(P(1)); put("X", a.X); put("Y", a.Y); });
    seg("ProjectivePoint::operator+", [] { put("ret", PJ(1) + PJ(2)); });
    seg("ProjectivePoint::double_", [] { put("ret", PJ(1).double_()); });
    seg("ProjectivePoint::to_extended", [] { put("ret", PJ(1).to_extended()); });
    seg("ProjectivePoint::neg", [] { put("ret", -PJ(1)); });
    seg("ProjectivePoint::operator-", [] { put("ret", PJ(1) - PJ(2)); });
    seg("ProjectivePoint::operator*", [] { put("ret", PJ(1) * S(2)); });
    seg("ProjectivePoint::operator==", [] { put("ret", PJ(1) == PJ(2)); });
    seg("ProjectivePoint::is_valid", [] { put("ret", PJ(1).is_valid()); });
    seg("coset4", [] { const auto c = coset4(P(1)); put("ret", std::vector<EdwardsPoint>(c.begin(), c.end())); });
    seg("CompressedEdwardsY::decompress", [] { CompressedEdwardsY c; c.bytes = B<32>(1); const auto r = c.decompress(); put("has", r.has_value()); if (r) put("ret", *r); });
    seg("mul_by_pow_2", [] { put("ret", mul_by_pow_2(P(1), 77)); });
    seg("mul_by_cofactor", [] { put("ret", mul_by_cofactor(P(1))); });
    seg("RistrettoPoint::operator==", [] { put("ret", RistrettoPoint{P(1)} == RistrettoPoint{P(2)}); });
    seg("RistrettoPoint::is_valid", [] { put("ret", RistrettoPoint{P(1)}.is_valid()); });
    seg("RistrettoPoint::elligator_ristretto_flavor", [] { put("ret", RistrettoPoint::elligator_ristretto_flavor(F(1)).p); });
    seg("RistrettoPoint::from_uniform_bytes", [] { put("ret", RistrettoPoint::from_uniform_bytes(B<64>(1)).p); });
    seg("RistrettoPoint::compress", [] { put("ret", RistrettoPoint{P(1)}.compress()); });
    seg("CompressedRistretto::decompress", [] { const auto r = E(1).decompress(); put("has", r.has_value()); if (r) put("ret", r->p); });

    // ---- the wrappers that pack rows: n in {0, 1, 3}, terms in {1, 2, 8}
    for (size_t n : {0, 1, 3}) {
        const std::string N = kv("n", n);
        seg("mul_batch" + N, [n] { put("ret", mul_batch(points(1, n), scalars(2, n))); });
        seg("mul_batch_fe" + N, [n] {
            std::vector<FieldElement> a, b;
            for (size_t i = 0; i < n; i++) { a.push_back(F(1, i)); b.push_back(F(2, i)); }
            put("ret", mul_batch(a, b));
        });
        seg("ristretto_roundtrip_mul_batch" + N, [n] {
            const auto r = ristretto_roundtrip_mul_batch(encs(1, n), scalars(2, n));
            std::vector<uint8_t> has;
            std::vector<CompressedRistretto> got;
            for (const auto& o : r) { has.push_back(o.has_value()); if (o) got.push_back(*o); }
            put("has", has);
            put("ret", got);
        });
        seg("msm" + N, [n] { put("ret", msm(points(1, n), scalars(2, n))); });
        seg("fold_ordered" + N, [n] { put("ret", fold_ordered(points(1, n))); });
        seg("msm_sharded" + N, [n] { put("ret", msm_sharded(points(1, n), scalars(2, n))); });
        seg("double_and_compress_batch" + N, [n] {
            std::vector<RistrettoPoint> ps;
            for (size_t i = 0; i < n; i++) ps.push_back({P(1, i)});
            put("ret", double_and_compress_batch(ps));
        });
        seg("mul_base_batch" + N, [n] { put("ret", mul_base_batch(scalars(1, n))); });
        seg("window_naf_mul_batch" + N + " width=6", [n] { put("ret", window_naf_mul_batch(scalars(1, n), 6)); });
        seg("ristretto_keygen_batch" + N, [n] { put("ret", ristretto_keygen_batch(scalars(1, n))); });
        seg("scalar_mul_shared" + N, [n] { put("ret", scalar_mul_shared(points(1, n), S(2))); });
        seg("ris_mul_shared" + N, [n] { const auto r = ris_mul_shared(encs(1, n), S(2)); put("ret", r.first); put("ok", r.second); });
        for (size_t t : {1, 2, 8}) {
            const std::string NT = N + kv("t", t);
            seg("ed_lincomb" + NT, [n, t] { put("ret", ed_lincomb(pt_rows(1, n, t), sc_rows(2, n, t))); });
            for (int bs = 0; bs < 2; bs++) {
                seg("ris_lincomb" + NT + kv("bs", bs), [n, t, bs] {
                    const auto r = bs ? ris_lincomb(enc_rows(1, n, t), sc_rows(2, n, t), scalars(3, n)) : ris_lincomb(enc_rows(1, n, t), sc_rows(2, n, t));
                    put("ret", r.first);
                    put("ok", r.second);
                });
                for (int zs = 0; zs < 2; zs++)
                    seg("ris_lincomb_sum" + NT + kv("bs", bs) + kv("zs", zs), [n, t, bs, zs] {
                        const auto r = ris_lincomb_sum(enc_rows(1, n, t), sc_rows(2, n, t), bs ? scalars(3, n) : std::vector<Scalar>{}, zs ? scalars(4, n) : std::vector<Scalar>{});
                        put("ret", r.first);
                        put("ok", r.second);
                    });
            }
            seg("ed_lincomb_shared" + NT, [n, t] { put("ret", ed_lincomb_shared(pt_rows(1, n, t), scalars(2, t))); });
            seg("ris_lincomb_shared" + NT, [n, t] { const auto r = ris_lincomb_shared(enc_rows(1, n, t), scalars(2, t)); put("ret", r.first); put("ok", r.second); });
        }
    }
    seg("msm_partial n=3", [] {
        std::vector<uint64_t> p(60), k(15), o(20);
        for (size_t i = 0; i < 3; i++) { P(1, i).flat(&p[20 * i]); std::memcpy(&k[5 * i], S(2, i).l.data(), 40); }
        msm_partial(p.data(), k.data(), 3, o.data());
        put_bytes("out_dev", o.data(), 160);
    });
    seg("msm_plan n=1000 aligned=1", [] { put("ret", msm_plan(1000)); });
    seg("msm_plan n=77 aligned=0", [] { put("ret", msm_plan(77, false)); });
    seg("msm_batch_plan n=100 batch=7 aligned=1", [] { put("ret", msm_batch_plan(100, 7)); });
    seg("msm_batch_plan n=9 batch=2 aligned=0", [] { put("ret", msm_batch_plan(9, 2, false)); });
    seg("MsmBases::plan n=500 window_bits=0", [] { put("ret", MsmBases::plan(500)); });
    seg("MsmBases::plan n=6 window_bits=9", [] { put("ret", MsmBases::plan(6, 9)); });
    for (size_t batch : {0, 2})
        for (size_t n : {0, 3})
            seg("msm_batch" + kv("batch", batch) + kv("n", n), [batch, n] { put("ret", msm_batch(pt_rows(1, batch, n), sc_rows(2, batch, n))); });

    // ---- MsmBases: 3 bases, one vector and two vectors of scalars, window_bits 0 and 9; the handle's life
    for (int wb : {0, 9})
        seg("MsmBases use" + kv("window_bits", (size_t)wb), [wb] {
            MsmBases t(points(1, 3), wb);
            put_int("size", (long long)t.size());
            put("one", t.msm(scalars(2, 3)));
            put("two", t.msm(sc_rows(3, 2, 3)));
            put("none", t.msm(ScRows{}));
        });
    seg("MsmBases move", [] {
        MsmBases a(points(1, 3));
        MsmBases b(std::move(a));                    // a destroys nothing
        put("moved", b.msm(scalars(2, 3)));
    });
    seg("MsmBases move_assign", [] {
        MsmBases a(points(1, 3)), b(points(2, 2));
        b = std::move(a);                            // destroys b's own table first
        put_int("size", (long long)b.size());
        put("assigned", b.msm(scalars(3, 3)));
    });

    // ---- Generators: 1, 2 and 8 generators x 3 rows (and no rows); the handle's life
    for (size_t count : {1, 2, 8})
        seg("Generators use" + kv("count", count), [count] {
            Generators g(points(1, count));
            put_int("size", (long long)g.size());
            put("mul", g.mul(sc_rows(2, 3, count)));
            put("mul_compress", g.mul_compress(sc_rows(3, 3, count)));
            put("mul0", g.mul(ScRows{}));
            put("mul_compress0", g.mul_compress(ScRows{}));
        });
    seg("Generators move", [] {
        Generators a(points(1, 2));
        Generators b(std::move(a));
        put("moved", b.mul(sc_rows(2, 3, 2)));
    });
    seg("Generators move_assign", [] {
        Generators a(points(1, 2)), b(points(2, 1));
        b = std::move(a);
        put_int("size", (long long)b.size());
        put("assigned", b.mul_compress(sc_rows(3, 3, 2)));
    });

    // ---- sum_rows: terms 0, 1, 3 and 33 x 3 rows (and no rows), both overloads, ok taken and not taken
    for (size_t n : {0, 3})
        for (size_t t : {0, 1, 3, 33}) {
            const std::string NT = kv("n", n) + kv("t", t);
            seg("sum_rows_ed" + NT, [n, t] { put("ret", sum_rows(pt_rows(1, n, t))); });
            seg("sum_rows_wire" + NT + " ok=0", [n, t] { put("ret", sum_rows(enc_rows(1, n, t))); });
            seg("sum_rows_wire" + NT + " ok=1", [n, t] {
                std::vector<uint8_t> ok(7, 9);
                put("ret", sum_rows(enc_rows(1, n, t), &ok));
                put("ok", ok);
            });
        }

    // ---- HashParts: 1 part and 4 parts of different row_bytes, prefix "" and a 3-byte prefix, 3 rows
    for (size_t nparts : {1, 4})
        for (size_t plen : {0, 3}) {
            const size_t row_bytes[4] = {1, 5, 130, 32};
            std::vector<std::vector<uint8_t>> bufs(nparts);
            HashParts parts;
            for (size_t j = 0; j < nparts; j++) {
                for (size_t i = 0; i < 3; i++)
                    for (size_t b = 0; b < row_bytes[j]; b++) bufs[j].push_back(byte_of(1, i, j, b));
                parts.add(bufs[j].data(), row_bytes[j]);
            }
            const std::string prefix = plen ? std::string("\x01pq", 3) : std::string();
            const std::string tag = kv("nparts", nparts) + kv("prefix", plen);
            seg("sha512_rows" + tag, [&] { std::vector<uint8_t> o(3 * 64); sha512_rows(prefix, parts, o.data(), 3); put("out", o); });
            seg("sc_from_sha512" + tag, [&] { std::vector<uint64_t> o(3 * 5); sc_from_sha512(prefix, parts, o.data(), 3); put_bytes("out", o.data(), 120); });
            seg("ris_from_sha512" + tag, [&] { std::vector<uint64_t> o(3 * 20); ris_from_sha512(prefix, parts, o.data(), 3); put_bytes("out", o.data(), 480); });
        }

    // ---- ragged rows and size mismatches: std::invalid_argument before anything reaches the library
    seg("mul_batch mismatch", [] { (void)mul_batch(points(1, 3), scalars(2, 2)); });
    seg("mul_batch_fe mismatch", [] { (void)mul_batch(std::vector<FieldElement>(3), std::vector<FieldElement>(2)); });
    seg("ristretto_roundtrip_mul_batch mismatch", [] { (void)ristretto_roundtrip_mul_batch(encs(1, 3), scalars(2, 2)); });
    seg("msm mismatch", [] { (void)msm(points(1, 3), scalars(2, 2)); });
    seg("msm_batch mismatch", [] { (void)msm_batch(pt_rows(1, 2, 3), sc_rows(2, 3, 3)); });
    seg("msm_batch ragged", [] { auto p = pt_rows(1, 2, 3); auto k = sc_rows(2, 2, 3); k[1].pop_back(); (void)msm_batch(p, k); });
    seg("ed_lincomb mismatch", [] { (void)ed_lincomb(pt_rows(1, 3, 2), sc_rows(2, 2, 2)); });
    seg("ed_lincomb ragged", [] { auto p = pt_rows(1, 3, 2); p[2].pop_back(); (void)ed_lincomb(p, sc_rows(2, 3, 2)); });
    seg("ris_lincomb mismatch", [] { (void)ris_lincomb(enc_rows(1, 3, 2), sc_rows(2, 3, 2), scalars(3, 2)); });
    seg("ris_lincomb ragged", [] { auto k = sc_rows(2, 3, 2); k[1].pop_back(); (void)ris_lincomb(enc_rows(1, 3, 2), k); });
    seg("ris_lincomb_sum mismatch", [] { (void)ris_lincomb_sum(enc_rows(1, 3, 2), sc_rows(2, 3, 2), {}, scalars(4, 4)); });
    seg("ris_lincomb_sum ragged", [] { auto e = enc_rows(1, 3, 2); e[0].pop_back(); (void)ris_lincomb_sum(e, sc_rows(2, 3, 2)); });
    seg("ed_lincomb_shared ragged", [] { auto p = pt_rows(1, 3, 2); p[1].pop_back(); (void)ed_lincomb_shared(p, scalars(2, 2)); });
    seg("ris_lincomb_shared ragged", [] { auto e = enc_rows(1, 3, 2); e[2].pop_back(); (void)ris_lincomb_shared(e, scalars(2, 2)); });
    seg("sum_rows_ed ragged", [] { auto p = pt_rows(1, 3, 3); p[1].pop_back(); (void)sum_rows(p); });
    seg("sum_rows_wire ragged", [] { auto e = enc_rows(1, 3, 3); e[2].pop_back(); (void)sum_rows(e); });
    seg("MsmBases ragged", [] { MsmBases t(points(1, 3)); auto k = sc_rows(2, 2, 3); k[1].pop_back(); (void)t.msm(k); });
    // the first row is the long one (rows 1 and 2 still differ from it: a check against the first row's length throws here too, and
    // is caught by "wrong_length" below, where every row has that length)
    seg("Generators ragged", [] { Generators g(points(1, 3)); auto k = sc_rows(2, 3, 3); k[0].push_back(S(2, 0, 3)); (void)g.mul(k); });
    seg("Generators wrong_length", [] { Generators g(points(1, 3)); (void)g.mul(sc_rows(2, 3, 4)); });      // every row of one length, not the set's
    seg("Generators ragged_compress", [] { Generators g(points(1, 3)); auto k = sc_rows(2, 3, 3); k[2].pop_back(); (void)g.mul_compress(k); });
    mark("exit");
    return 0;
}
