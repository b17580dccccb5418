// C++ host-mirror tests, second program: every wrapper of zerocaf.hpp that tests/cpp/test_zerocaf_hpp.cpp does not run, at the
// smallest shapes that can still be wrong, against the composition of the operators that program pins to the reference's known
// answers (operator*, operator+, compress, decompress, Scalar arithmetic).  Needs a GPU.  Prints "ran <wrapper> <shapes>" per
// wrapper, "plan ..." lines that tests/test_gpu_cpp_mirror.py compares with the Python Engine's, and "all extended checks passed".
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include "../../dusk_zerocaf_amd/include/zerocaf.hpp"

#include <hip/hip_runtime_api.h>         // hipMalloc / hipMemcpy / hipFree for msm_partial's device buffer (-D__HIP_PLATFORM_AMD__)

using namespace zerocaf;
static int failures = 0;
#define CHECK(...) do { if (!(__VA_ARGS__)) { std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #__VA_ARGS__); failures++; } } while (0)
typedef std::array<uint64_t, 5> L5;
typedef std::vector<std::vector<EdwardsPoint>> PtRows;
typedef std::vector<std::vector<Scalar>> ScRows;
typedef std::vector<std::vector<CompressedRistretto>> EncRows;
static const size_t TERMS[3] = {1, 2, 8};

static bool limbs_equal(const EdwardsPoint& a, const EdwardsPoint& b) { return a.X.l == b.X.l && a.Y.l == b.Y.l && a.Z.l == b.Z.l && a.T.l == b.T.l; }
// the same group element: == (affine) and identical compress() bytes
static bool same(const EdwardsPoint& a, const EdwardsPoint& b) { return a == b && a.compress().bytes == b.compress().bytes; }
static bool zero32(const CompressedRistretto& c) { for (uint8_t b : c.bytes) if (b) return false; return true; }
static EdwardsPoint fold(const std::vector<EdwardsPoint>& ps, const std::vector<Scalar>& ks)          // ((k0*P0 + k1*P1) + ...)
{
    EdwardsPoint acc = ps[0] * ks[0];
    for (size_t j = 1; j < ps.size(); j++) acc = acc + ps[j] * ks[j];
    return acc;
}
static EdwardsPoint sum(const std::vector<EdwardsPoint>& ps)
{
    EdwardsPoint acc = EdwardsPoint::identity();
    for (const EdwardsPoint& p : ps) acc = acc + p;
    return acc;
}
// compress(b * B + sum_j k_j * decompress(e_j)) through RistrettoPoint; nothing where a term does not decode
static std::optional<RistrettoPoint> wire_sum(const std::vector<CompressedRistretto>& es, const std::vector<Scalar>& ks, const Scalar* b)
{
    RistrettoPoint acc = RistrettoPoint::identity();
    for (size_t j = 0; j < es.size(); j++) {
        const auto p = es[j].decompress();
        if (!p) return std::nullopt;
        acc = acc + *p * ks[j];
    }
    if (b) acc = acc + constants::RISTRETTO_BASEPOINT() * *b;
    return acc;
}
// a row of the wire-format wrappers: mask and bytes against the composition (mask 0 and 32 zero bytes where a term does not decode)
static bool wire_row_ok(const CompressedRistretto& got, uint8_t ok, const std::optional<RistrettoPoint>& want)
{
    if (!want) return ok == 0 && zero32(got);
    return ok == 1 && got == want->compress();
}
static std::array<uint8_t, 64> hex64(const char* h)
{
    std::array<uint8_t, 64> b{};
    for (int i = 0; i < 64; i++) { unsigned v; std::sscanf(h + 2 * i, "%2x", &v); b[i] = (uint8_t)v; }
    return b;
}
template <class F>
static bool throws_runtime_error(F f)
{
    try { f(); } catch (const std::runtime_error&) { return true; }
    return false;
}

int main()
{
    const EdwardsPoint Bp = constants::BASEPOINT();
    const RistrettoPoint RB = constants::RISTRETTO_BASEPOINT();
    const EdwardsPoint ID = EdwardsPoint::identity();
    const EdwardsPoint P1{FieldElement(L5{13, 0, 0, 0, 0}),
                          FieldElement(L5{606320128494542ull, 1597163540666577ull, 1835599237877421ull, 1667478411389512ull, 3232679738299ull}),
                          FieldElement::one(),
                          FieldElement(L5{2034732376387996ull, 3922598123714460ull, 1344791952818393ull, 3662820838581677ull, 6840464509059ull})};
    const EdwardsPoint P2{FieldElement(L5{67, 0, 0, 0, 0}),
                          FieldElement(L5{2369245568431362ull, 2665603790611352ull, 3317390952748653ull, 1908583331312524ull, 8011773354506ull}),
                          FieldElement::one(),
                          FieldElement(L5{3474019263728064ull, 2548729061993416ull, 1588812051971430ull, 1774293631565269ull, 9023233419450ull})};
    const Scalar Y(L5{138340288859536ull, 461913478537005ull, 1182880083788836ull, 1688835920473363ull, 1743782656037ull});     // canonical (scalar.rs KATs)
    const Scalar M1 = Scalar::minus_one();
    // small multiples of the basepoint and their encodings: Bm[m] = m * B by repeated addition, Em[0] = the identity's zero bytes
    std::vector<EdwardsPoint> Bm = {ID};
    for (int m = 1; m <= 40; m++) Bm.push_back(Bm.back() + Bp);
    std::vector<CompressedRistretto> Em;
    for (const EdwardsPoint& p : Bm) Em.push_back(RistrettoPoint{p}.compress());
    CompressedRistretto BAD;                                      // an encoding that does not decode
    BAD.bytes.fill(0xff);
    CHECK(!BAD.decompress().has_value() && zero32(Em[0]) && Em[5].decompress().has_value());
    // element (row i, term j) of the inputs: points among m * B, P1, P2 and the identity, scalars small, large and -1
    const auto pt = [&](size_t i, size_t j) -> EdwardsPoint {
        if (i == 1 && j == 0) return ID;                          // one row holds the identity
        if ((i + j) % 4 == 1) return P1;
        if ((i + j) % 4 == 3) return P2;
        return Bm[1 + 3 * i + j];
    };
    const auto enc = [&](size_t i, size_t j) -> CompressedRistretto { return (i == 1 && j == 0) ? Em[0] : Em[2 + 5 * i + j]; };
    const auto sc = [&](size_t i, size_t j) -> Scalar {
        if ((i + 2 * j) % 5 == 1) return Y;
        if ((i + 2 * j) % 5 == 3) return M1;
        if (i == 2 && j == 1) return Scalar::zero();
        return Scalar(1000 * i + 7 * j + 2);
    };
    const auto pt_rows = [&](size_t n, size_t t) { PtRows r(n); for (size_t i = 0; i < n; i++) for (size_t j = 0; j < t; j++) r[i].push_back(pt(i, j)); return r; };
    const auto sc_rows = [&](size_t n, size_t t) { ScRows r(n); for (size_t i = 0; i < n; i++) for (size_t j = 0; j < t; j++) r[i].push_back(sc(i, j)); return r; };
    // the wire rows: row `bad_row` (if < n) holds the undecodable encoding in its last term
    const auto enc_rows = [&](size_t n, size_t t, size_t bad_row) {
        EncRows r(n);
        for (size_t i = 0; i < n; i++) for (size_t j = 0; j < t; j++) r[i].push_back(i == bad_row && j == t - 1 ? BAD : enc(i, j));
        return r;
    };
    const size_t NO_BAD = 99;

    // ---- fold_ordered, msm_partial, msm_batch
    {
        const std::vector<EdwardsPoint> ps = {P1, ID, Bm[7], P2};
        CHECK(same(fold_ordered(ps), ((P1 + ID) + Bm[7]) + P2));
        CHECK(limbs_equal(fold_ordered({P2}), P2) || same(fold_ordered({P2}), P2));
        CHECK(throws_runtime_error([] { (void)fold_ordered({}); }));                      // the library refuses an empty list (as for the Engine)
        std::printf("ran fold_ordered count=4,1,0\n");

        const std::vector<Scalar> ks = {Scalar(5), Y, M1, Scalar(77)};
        std::vector<uint64_t> p(80), k(20), o(20, 0);
        for (size_t i = 0; i < 4; i++) { ps[i].flat(&p[20 * i]); std::memcpy(&k[5 * i], ks[i].l.data(), 40); }
        void* dev = nullptr;
        CHECK(hipMalloc(&dev, 160) == hipSuccess && dev != nullptr);
        if (dev) {
            msm_partial(p.data(), k.data(), 4, static_cast<uint64_t*>(dev));
            Backend::synchronize();
            CHECK(hipMemcpy(o.data(), dev, 160, hipMemcpyDeviceToHost) == hipSuccess);
            CHECK(same(EdwardsPoint::unflat(o.data()), fold(ps, ks)));
            msm_partial(p.data(), k.data(), 0, static_cast<uint64_t*>(dev));              // no pairs: the identity
            Backend::synchronize();
            CHECK(hipMemcpy(o.data(), dev, 160, hipMemcpyDeviceToHost) == hipSuccess);
            CHECK(limbs_equal(EdwardsPoint::unflat(o.data()), ID));
            CHECK(hipFree(dev) == hipSuccess);
        }
        std::printf("ran msm_partial n=4,0\n");

        CHECK(limbs_equal(msm({}, {}), ID));                                              // the empty sum
        const PtRows pss = {{P1, Bm[3], ID}, {P2, P1, Bm[9]}};
        const ScRows kss = {{Y, Scalar(6), Scalar(9)}, {M1, Scalar::zero(), Scalar(123456789)}};
        const auto got = msm_batch(pss, kss);
        CHECK(got.size() == 2);
        for (size_t b = 0; b < got.size(); b++) CHECK(same(got[b], fold(pss[b], kss[b])));
        CHECK(msm_batch({}, {}).empty());
        const auto idents = msm_batch(PtRows(2), ScRows(2));                              // instances of no pairs
        CHECK(idents.size() == 2 && limbs_equal(idents[0], ID) && limbs_equal(idents[1], ID));
        std::printf("ran msm_batch batch=2 n=3; batch=0; batch=2 n=0\n");
    }

    // ---- plans: printed, compared with the Python Engine's by the test
    for (const auto& nb : std::vector<std::pair<size_t, size_t>>{{3, 2}, {64, 100}, {4096, 8}}) {
        const auto v = msm_batch_plan(nb.first, nb.second);
        std::printf("plan msm_batch %zu %zu", nb.first, nb.second);
        for (int32_t x : v) std::printf(" %d", x);
        std::printf("\n");
    }
    for (const auto& nw : std::vector<std::pair<size_t, int>>{{3, 0}, {3, 9}, {5000, 0}}) {
        const auto v = MsmBases::plan(nw.first, nw.second);
        std::printf("plan msm_fixed %zu %d", nw.first, nw.second);
        for (int32_t x : v) std::printf(" %d", x);
        std::printf("\n");
    }

    // ---- double_and_compress_batch, window_naf_mul_batch
    {
        const std::vector<EdwardsPoint> ps = {Bm[3], ID, P1, Bm[11]};
        std::vector<RistrettoPoint> rs;
        for (const auto& p : ps) rs.push_back({p});
        const auto got = double_and_compress_batch(rs);
        CHECK(got.size() == 4);
        for (size_t i = 0; i < got.size(); i++) CHECK(got[i] == RistrettoPoint{ps[i].double_()}.compress());
        CHECK(zero32(got[1]));
        CHECK(double_and_compress_batch({}).empty());
        std::printf("ran double_and_compress_batch n=4,0\n");
        const std::vector<Scalar> ks = {Scalar(1), Scalar::zero(), Y, Scalar(12345)};
        for (unsigned w : {2u, 7u}) {
            const auto out = window_naf_mul_batch(ks, w);
            CHECK(out.size() == 4);
            for (size_t i = 0; i < out.size(); i++) CHECK(same(out[i], Bp * ks[i]));
            CHECK(window_naf_mul_batch({}, w).empty());
        }
        std::printf("ran window_naf_mul_batch n=4,0 width=2,7\n");
        CHECK(mul_batch(std::vector<EdwardsPoint>{}, std::vector<Scalar>{}).empty() && mul_batch(std::vector<FieldElement>{}, std::vector<FieldElement>{}).empty());
        CHECK(mul_base_batch({}).empty() && ristretto_keygen_batch({}).empty() && ristretto_roundtrip_mul_batch({}, {}).empty());
        std::printf("ran mul_batch, mul_base_batch, ristretto_keygen_batch, ristretto_roundtrip_mul_batch n=0\n");
    }

    // ---- ed_lincomb, ed_lincomb_shared, ris_lincomb, ris_lincomb_shared, ris_lincomb_sum: 3 rows (and none), terms 1, 2, 8
    for (size_t t : TERMS) {
        const PtRows pss = pt_rows(3, t);
        const ScRows kss = sc_rows(3, t);
        const auto got = ed_lincomb(pss, kss);
        CHECK(got.size() == 3);
        for (size_t i = 0; i < got.size(); i++) CHECK(same(got[i], fold(pss[i], kss[i])));
        const auto shared = ed_lincomb_shared(pss, kss[0]);
        CHECK(shared.size() == 3);
        for (size_t i = 0; i < shared.size(); i++) CHECK(same(shared[i], fold(pss[i], kss[0])));
        CHECK(ed_lincomb({}, {}).empty() && ed_lincomb_shared({}, kss[0]).empty());

        const std::vector<Scalar> bs = {Scalar(3), Y, M1};
        for (size_t bad_row : {NO_BAD, (size_t)1}) {
            const EncRows ess = enc_rows(3, t, bad_row);
            for (int with_bs = 0; with_bs < 2; with_bs++) {
                if (with_bs && t == 8) continue;                                              // the base term takes one of the eight slots
                const auto r = with_bs ? ris_lincomb(ess, kss, bs) : ris_lincomb(ess, kss);
                CHECK(r.first.size() == 3 && r.second.size() == 3);
                for (size_t i = 0; i < r.first.size(); i++) {
                    CHECK(wire_row_ok(r.first[i], r.second[i], wire_sum(ess[i], kss[i], with_bs ? &bs[i] : nullptr)));
                    CHECK((r.second[i] == 0) == (i == bad_row));                          // exactly the row with the bad encoding
                }
            }
            const auto s = ris_lincomb_shared(ess, kss[1]);
            CHECK(s.first.size() == 3 && s.second.size() == 3);
            for (size_t i = 0; i < s.first.size(); i++) {
                CHECK(wire_row_ok(s.first[i], s.second[i], wire_sum(ess[i], kss[1], nullptr)));
                CHECK((s.second[i] == 0) == (i == bad_row));
            }
            // the weighted sum of all rows: w_ij = z_i k_ij, b = sum z_i b_i, built from Scalar products; a bad row is left out
            const std::vector<Scalar> zs = {Scalar(11), Y, Scalar(2)};
            for (int with_bs = 0; with_bs < 2; with_bs++)
                for (int with_zs = 0; with_zs < 2; with_zs++) {
                    const auto r = ris_lincomb_sum(ess, kss, with_bs ? bs : std::vector<Scalar>{}, with_zs ? zs : std::vector<Scalar>{});
                    RistrettoPoint want = RistrettoPoint::identity();
                    for (size_t i = 0; i < 3; i++) {
                        CHECK((r.second[i] == 0) == (i == bad_row));
                        if (i == bad_row) continue;
                        std::vector<Scalar> w;
                        for (size_t j = 0; j < t; j++) w.push_back(with_zs ? zs[i] * kss[i][j] : kss[i][j]);
                        const Scalar b = with_zs ? zs[i] * bs[i] : bs[i];
                        want = want + *wire_sum(ess[i], w, with_bs ? &b : nullptr);
                    }
                    CHECK(r.second.size() == 3 && r.first == want.compress());
                }
        }
        CHECK(ris_lincomb({}, {}).first.empty() && ris_lincomb({}, {}).second.empty());
        CHECK(ris_lincomb_shared({}, kss[0]).first.empty());
        const auto none = ris_lincomb_sum({}, {});                                            // the empty sum: the identity's encoding
        CHECK(zero32(none.first) && none.second.empty());
    }
    std::printf("ran ed_lincomb, ed_lincomb_shared n=3,0 terms=1,2,8\n");
    std::printf("ran ris_lincomb n=3,0 terms=1,2,8 (with bs: 1,2); ris_lincomb_shared n=3,0 terms=1,2,8; each with and without an undecodable term in row 1\n");
    std::printf("ran ris_lincomb_sum n=3,0 terms=1,2,8 with and without bs and zs, with and without an undecodable term in row 1\n");

    // ---- ris_lincomb_sum on a Schnorr batch: sum_i z_i (s_i B - c_i A_i - R_i) = 0 for three valid signatures
    {
        EncRows ess;
        ScRows kss;
        std::vector<Scalar> ss, zs = {Scalar(1), Y, Scalar(987654321)};
        for (uint64_t i = 0; i < 3; i++) {
            const Scalar x = Scalar(1000 + i) * Y, r = Scalar(31 + i) + Y, c = Scalar(7 + 5 * i) * Y.square();
            ess.push_back({(RB * x).compress(), (RB * r).compress()});
            kss.push_back({-c, M1});
            ss.push_back(r + c * x);
        }
        const auto v = ris_lincomb_sum(ess, kss, ss, zs);
        CHECK(zero32(v.first) && v.second == std::vector<uint8_t>({1, 1, 1}));
        ss[1] = ss[1] + Scalar::one();                                                        // a forged signature: not the identity
        CHECK(!zero32(ris_lincomb_sum(ess, kss, ss, zs).first));
        std::printf("ran ris_lincomb_sum schnorr n=3 terms=2\n");
    }

    // ---- scalar_mul_shared, ris_mul_shared
    {
        const std::vector<EdwardsPoint> ps = {P1, ID, Bm[9]};
        for (const Scalar& k : {Y, Scalar(6), M1}) {
            const auto got = scalar_mul_shared(ps, k);
            CHECK(got.size() == 3);
            for (size_t i = 0; i < got.size(); i++) CHECK(same(got[i], ps[i] * k));
            const std::vector<CompressedRistretto> es = {Em[4], BAD, Em[0]};
            const auto r = ris_mul_shared(es, k);
            CHECK(r.first.size() == 3 && r.second == std::vector<uint8_t>({1, 0, 1}));
            for (size_t i = 0; i < r.first.size(); i++) CHECK(wire_row_ok(r.first[i], r.second[i], wire_sum({es[i]}, {k}, nullptr)));
        }
        CHECK(scalar_mul_shared({}, Y).empty() && ris_mul_shared({}, Y).first.empty() && ris_mul_shared({}, Y).second.empty());
        std::printf("ran scalar_mul_shared, ris_mul_shared n=3,0\n");
    }

    // ---- HashParts: sha512_rows against digests made with Python's hashlib when this file was written; row 0 of the first two
    //      cases is the FIPS 180-4 "abc" vector ("ab" as the prefix and "c" as the part -- a part has at least one byte -- and
    //      "abc" as a part); the third case spans two blocks (171 bytes a row)
    {
        static const char* want[3][3] = {
            {"ddaf35a193617abacc417349ae20413112e6fa4e89a97ea20a9eeee64b55d39a2192992a274fc1a836ba3c23a3feebbd454d4423643ce80e2a9ac94fa54ca49f",
             "1a9840c27a5cf22dab060cdd8a83da2b0fbcb1aeb52d4f9d3894b639083e205a5ab3f6afaeeb21b8e99b5e0fe93daafaabeef274da5d6eadcc9db36e5b6f64c4",
             "5861a8e5b486be0c5c0295b5430f74d475564c5028bebad286e950ed6c7095d67d022ad4f9455df419296b4e76f3a8bc642afc57e9791874ed1072b45cbd65a7"},
            {"ddaf35a193617abacc417349ae20413112e6fa4e89a97ea20a9eeee64b55d39a2192992a274fc1a836ba3c23a3feebbd454d4423643ce80e2a9ac94fa54ca49f",
             "1a9840c27a5cf22dab060cdd8a83da2b0fbcb1aeb52d4f9d3894b639083e205a5ab3f6afaeeb21b8e99b5e0fe93daafaabeef274da5d6eadcc9db36e5b6f64c4",
             "4a3ed8147e37876adc8f76328e5abcc1b470e6acfc18efea0135f983604953a58e183c1a6086e91ba3e821d926f5fdeb37761c7ca0328a963f5e92870675b728"},
            {"c3169c2f1a0e3207a5610a539b0c04d71ee3dc05022458c247d596ed4781f2df9ad953ac2f8695b2d45156bb9da9d843b1d972af2559056ae4b4c1d905d0aca3",
             "f8e7153656b51475e73b65bd1bea143ea295ed9b390f9cff5a727949cdc36759d67c78a4efb46fd4757449c6790659d2d8605515701335b9df3ba343071e8ca0",
             "a54739881ffbe891411c232369dff6c59128ccf0d94b2bf604c22f15f76e7f25fa85b3664294bd80df601363413c5deeed3599c4248ebbaf359db78116a143c4"}};
        const size_t row_bytes[4] = {1, 5, 130, 32};
        for (int c = 0; c < 3; c++) {
            std::string prefix;
            std::vector<std::vector<uint8_t>> bufs;
            if (c == 0) { prefix = "ab"; bufs = {{'c', 'd', 'e'}}; }
            if (c == 1) { bufs = {{'a', 'b', 'c', 'a', 'b', 'd', 'x', 'y', 'z'}}; }
            if (c == 2) {
                prefix = std::string("\x01pq", 3);
                bufs.resize(4);
                for (size_t j = 0; j < 4; j++)
                    for (size_t i = 0; i < 3; i++)
                        for (size_t b = 0; b < row_bytes[j]; b++) bufs[j].push_back((uint8_t)((i * 37 + j * 11 + b * 3 + 1) & 255));
            }
            HashParts parts;
            for (const auto& buf : bufs) parts.add(buf.data(), buf.size() / 3);
            std::vector<uint8_t> out(3 * 64);
            std::vector<uint64_t> s(3 * 5), g(3 * 20);
            sha512_rows(prefix, parts, out.data(), 3);
            sc_from_sha512(prefix, parts, s.data(), 3);
            ris_from_sha512(prefix, parts, g.data(), 3);
            for (size_t i = 0; i < 3; i++) {
                const std::array<uint8_t, 64> d = hex64(want[c][i]);
                CHECK(std::memcmp(&out[64 * i], d.data(), 64) == 0);
                CHECK(std::memcmp(&s[5 * i], Scalar::from_bytes_wide(d).l.data(), 40) == 0);          // the wide reduction of the digest
                CHECK(limbs_equal(EdwardsPoint::unflat(&g[20 * i]), RistrettoPoint::from_uniform_bytes(d).p));   // limb for limb
            }
            std::vector<uint8_t> untouched(64, 0x5a);
            sha512_rows(prefix, parts, untouched.data(), 0);                                      // no rows: nothing written
            CHECK(untouched == std::vector<uint8_t>(64, 0x5a));
        }
        std::printf("ran sha512_rows, sc_from_sha512, ris_from_sha512 n=3,0 parts=1,1,4 prefix=2,0,3 bytes (one case of two blocks)\n");
    }

    // ---- the scalar extensions against Scalar *, + and pow
    {
        std::array<uint8_t, 64> wide{};
        for (int i = 0; i < 64; i++) wide[i] = (uint8_t)(251 - 3 * i);
        std::array<uint8_t, 32> lo{}, hi{}, ones{};
        std::memcpy(lo.data(), wide.data(), 32);
        std::memcpy(hi.data(), wide.data() + 32, 32);
        ones.fill(0xff);
        const auto horner = [](const std::array<uint8_t, 32>& b) {                            // sum b_i 256^i from Scalar * and +
            Scalar acc = Scalar::zero();
            for (int i = 31; i >= 0; i--) acc = acc * Scalar(256) + Scalar(b[i]);
            return acc;
        };
        CHECK(Scalar::from_bytes_mod_order(lo).l == horner(lo).l && Scalar::from_bytes_mod_order(ones).l == horner(ones).l);
        CHECK(Scalar::from_bytes_mod_order(Y.to_bytes()).l == Y.l);
        const Scalar two256 = Scalar::two_pow_k(128) * Scalar::two_pow_k(128);
        CHECK(Scalar::from_bytes_wide(wide).l == (horner(lo) + horner(hi) * two256).l);
        CHECK(Y.muladd(M1, Scalar(99)).l == (Y * M1 + Scalar(99)).l && Scalar(5).muladd(Scalar(6), Scalar(7)).l == Scalar(37).l);
        const Scalar l_minus_2 = M1 - Scalar::one();
        CHECK(Y.invert().l == Y.pow(l_minus_2).l && (Y.invert() * Y).l == Scalar::one().l && (Scalar(2).invert() * Scalar(2)).l == Scalar::one().l);
        bool threw = false;
        try { (void)Scalar::zero().invert(); } catch (const std::domain_error&) { threw = true; }
        CHECK(threw);
        std::printf("ran Scalar::from_bytes_wide, from_bytes_mod_order, muladd, invert\n");
    }

    // ---- MsmBases: 3 bases, one vector and two vectors of scalars, window_bits 0 and 9, two live tables used alternately
    {
        const std::vector<EdwardsPoint> bases_a = {Bp, P1, P2}, bases_b = {P2, ID, Bm[5]};
        const ScRows kss = {{Y, Scalar(6), M1}, {Scalar::zero(), Scalar(123456789), Y}};
        auto a = std::make_unique<MsmBases>(bases_a);
        MsmBases b(bases_b, 9);
        CHECK(a->size() == 3 && b.size() == 3);
        for (int round = 0; round < 2; round++) {
            CHECK(same(a->msm(kss[0]), fold(bases_a, kss[0])));
            CHECK(same(b.msm(kss[0]), fold(bases_b, kss[0])));
            const auto two_a = a->msm(kss), two_b = b.msm(kss);
            CHECK(two_a.size() == 2 && two_b.size() == 2);
            for (size_t v = 0; v < 2; v++) CHECK(same(two_a[v], fold(bases_a, kss[v])) && same(two_b[v], fold(bases_b, kss[v])));
        }
        CHECK(b.msm(ScRows{}).empty());
        a.reset();                                                                            // one goes, the other is still right
        CHECK(same(b.msm(kss[1]), fold(bases_b, kss[1])));
        MsmBases c(bases_a, 9);
        c = std::move(b);                                                                     // c's own table is destroyed first
        CHECK(same(c.msm(kss[1]), fold(bases_b, kss[1])));
        std::printf("ran MsmBases n=3 window_bits=0,9 batch=1,2,0\n");
    }

    // ---- Generators: 1, 2 and 8 generators x 3 rows (and none), two live sets used alternately, a point off the curve
    {
        const std::vector<std::vector<EdwardsPoint>> sets = {{P1}, {Bp, P2}, {Bm[1], Bm[2], P1, Bm[4], P2, Bm[6], Bm[7], ID}};
        const std::vector<std::vector<EdwardsPoint>> wire_sets = {{Bm[3]}, {Bp, Bm[9]}, {Bm[1], Bm[2], Bm[3], Bm[4], Bm[5], Bm[6], Bm[7], Bm[8]}};
        for (size_t s = 0; s < sets.size(); s++) {
            const size_t count = sets[s].size();
            const ScRows kss = sc_rows(3, count);
            Generators g(sets[s]), w(wire_sets[s]);
            CHECK(g.size() == count);
            for (int round = 0; round < 2; round++) {
                const auto got = g.mul(kss);
                const auto wire = w.mul_compress(kss);
                CHECK(got.size() == 3 && wire.size() == 3);
                for (size_t i = 0; i < 3; i++) {
                    CHECK(same(got[i], fold(sets[s], kss[i])));
                    CHECK(wire[i] == RistrettoPoint{fold(wire_sets[s], kss[i])}.compress());
                }
            }
            CHECK(g.mul(ScRows{}).empty() && g.mul_compress(ScRows{}).empty());
        }
        auto first = std::make_unique<Generators>(sets[1]);
        Generators second(sets[0]);
        const ScRows k2 = sc_rows(3, 2), k1 = sc_rows(3, 1);
        CHECK(same(first->mul(k2)[2], fold(sets[1], k2[2])) && same(second.mul(k1)[2], fold(sets[0], k1[2])));
        first.reset();
        CHECK(same(second.mul(k1)[0], fold(sets[0], k1[0])));
        Generators third(sets[1]);
        third = std::move(second);                                                            // third's own set is destroyed first
        CHECK(third.size() == 1 && same(third.mul(k1)[1], fold(sets[0], k1[1])));
        CHECK(throws_runtime_error([&] { Generators off(std::vector<EdwardsPoint>{EdwardsPoint{P1.X, P1.Y + FieldElement::one(), P1.Z, P1.T}}); }));
        std::printf("ran Generators count=1,2,8 n=3,0\n");
    }

    // ---- sum_rows: terms 1, 3 and 33 x 3 rows (and terms 0, and no rows), both overloads
    for (size_t t : {1, 3, 33}) {
        PtRows rows(3);
        EncRows wire(3);
        for (size_t i = 0; i < 3; i++)
            for (size_t j = 0; j < t; j++) {
                rows[i].push_back(j % 11 == 4 ? P1 : j % 11 == 9 ? P2 : (i == 1 && j == 0) ? ID : Bm[(i + j) % 40 + 1]);
                wire[i].push_back((i == 1 && j == 0) ? Em[0] : (i == 2 && j == t - 1) ? BAD : Em[(3 * i + j) % 40 + 1]);
            }
        const auto got = sum_rows(rows);
        CHECK(got.size() == 3);
        for (size_t i = 0; i < 3; i++) CHECK(same(got[i], sum(rows[i])));
        std::vector<uint8_t> ok;
        const auto enc_sum = sum_rows(wire, &ok);
        CHECK(enc_sum.size() == 3 && ok == std::vector<uint8_t>({1, 1, 0}));
        for (size_t i = 0; i < 3; i++) CHECK(wire_row_ok(enc_sum[i], ok[i], wire_sum(wire[i], std::vector<Scalar>(t, Scalar::one()), nullptr)));
        const auto untaken = sum_rows(wire);                                                  // the mask not taken
        CHECK(untaken == enc_sum);
    }
    {
        const auto e0 = sum_rows(PtRows(2));                                                  // rows of no terms: identities
        CHECK(e0.size() == 2 && same(e0[0], ID) && same(e0[1], ID));
        std::vector<uint8_t> ok(5, 9);
        const auto w0 = sum_rows(EncRows(2), &ok);
        CHECK(w0.size() == 2 && zero32(w0[0]) && zero32(w0[1]) && ok == std::vector<uint8_t>({1, 1}));
        CHECK(sum_rows(PtRows{}).empty() && sum_rows(EncRows{}, &ok).empty() && ok.empty());
        std::printf("ran sum_rows (both overloads) n=3 terms=1,3,33; n=2 terms=0; n=0\n");
    }

    // ---- the stream and buffer members of Backend (the communicator needs several ranks: tests/test_multi_gpu_rccl.py)
    {
        Backend::set_stream(nullptr);                                                         // the HIP null stream, as the caller's
        CHECK(same(mul_base_batch({Scalar(9)})[0], Bm[9]));
        Backend::synchronize();
        Backend::use_own_stream();
        Backend::set_stream_dev(0, nullptr);
        CHECK(same(scalar_mul_shared({Bp}, Scalar(7))[0], Bm[7]));
        Backend::use_own_stream();
        std::vector<uint64_t> pinned(4 * 20);
        Backend::host_register(pinned.data(), pinned.size() * 8);
        for (size_t i = 0; i < 4; i++) Bm[i + 1].flat(&pinned[20 * i]);
        uint64_t o[20];
        Backend::check(zc_ed_fold_ordered(Backend::ctx(), pinned.data(), 4, o), "zc_ed_fold_ordered");
        CHECK(same(EdwardsPoint::unflat(o), Bm[10]));
        Backend::host_unregister(pinned.data());
        CHECK(Backend::comm_size() == 0);                                                     // no communicator
        std::printf("ran Backend::set_stream, use_own_stream, set_stream_dev, host_register, host_unregister, comm_size\n");
    }
    Backend::synchronize();
    if (failures) { std::printf("%d FAILURES\n", failures); return 1; }
    std::printf("zerocaf.hpp: all extended checks passed\n");
    return 0;
}
