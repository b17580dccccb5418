// scalar_ext_san.cpp -- TEST-ONLY stand-alone program: replays a vector file through the host build of the scalar operations
// for protocols (scalar_ext_emul.cpp) and compares every row with the expected values the file carries.  Built with
// -fsanitize=address,undefined -fno-sanitize-recover=all by tests/test_scalar_ext_emul.py and run as a child process: the exit
// status is the verdict (0: every row matched and no sanitizer report; 1: a mismatch; 2: a malformed file).
//
// The file is a sequence of records of little-endian 64-bit words: op, n, c, then the inputs and the expected outputs, every
// array padded to a multiple of 8 bytes.  op 1: wide reduction (n x 64 bytes -> n x 5), 2: 32-byte reduction (n x 32 bytes),
// 3: muladd (a, b, c: n x 5 each), 4: one inversion per row (n x 5 -> n x 5 and n ok bytes), 5 / 6: shared inversions with
// chunk c on the column-ordered / independent-chain multiplier, 0: end.
#include <fstream>
#include <iterator>
#include <vector>
#include "scalar_ext_emul.cpp"

namespace {
struct Reader {
    std::vector<uint8_t> buf;
    size_t pos = 0;
    bool bad = false;
    const uint8_t* take(size_t bytes)
    {
        const size_t padded = (bytes + 7) & ~(size_t)7;
        if (padded > buf.size() - pos) {
            bad = true;
            return nullptr;
        }
        const uint8_t* p = buf.data() + pos;
        pos += padded;
        return p;
    }
    u64 word()
    {
        const uint8_t* p = take(8);
        u64 w = 0;
        if (p) std::memcpy(&w, p, 8);
        return w;
    }
    // a copy of exactly `bytes` bytes in a heap block of its own, so that a read past the end is an AddressSanitizer report
    template <class T>
    std::vector<T> array(size_t count)
    {
        std::vector<T> v(count);
        const uint8_t* p = take(count * sizeof(T));
        if (p && count) std::memcpy(v.data(), p, count * sizeof(T));
        return v;
    }
};

int compare(const char* what, u64 rec, const std::vector<u64>& got, const std::vector<u64>& want, const std::vector<uint8_t>* gok,
            const std::vector<uint8_t>* wok)
{
    for (size_t i = 0; i < want.size(); i++)
        if (got[i] != want[i]) {
            std::fprintf(stderr, "record %llu (%s): row %zu limb %zu: got %llx, want %llx\n", (unsigned long long)rec, what, i / 5, i % 5,
                         (unsigned long long)got[i], (unsigned long long)want[i]);
            return 1;
        }
    if (gok)
        for (size_t i = 0; i < wok->size(); i++)
            if ((*gok)[i] != (*wok)[i]) {
                std::fprintf(stderr, "record %llu (%s): row %zu: ok %d, want %d\n", (unsigned long long)rec, what, i, (*gok)[i], (*wok)[i]);
                return 1;
            }
    return 0;
}
}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) return 2;
    Reader r;
    r.buf.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    size_t rows = 0;
    for (u64 rec = 0;; rec++) {
        const u64 op = r.word(), n = r.word(), c = r.word();
        if (r.bad || op > 6 || n > (1u << 20)) return 2;
        if (op == 0) break;
        std::vector<u64> got(5 * n);
        int rc = 0;
        if (op == 1 || op == 2) {
            const auto in = r.array<uint8_t>((op == 1 ? 64 : 32) * n);
            const auto want = r.array<u64>(5 * n);
            if (r.bad) return 2;
            if (op == 1) emul_sc_from_bytes_wide(in.data(), got.data(), n);
            else emul_sc_from_bytes_mod_order(in.data(), got.data(), n);
            rc = compare(op == 1 ? "wide" : "mod_order", rec, got, want, nullptr, nullptr);
        } else if (op == 3) {
            const auto a = r.array<u64>(5 * n), b = r.array<u64>(5 * n), cc = r.array<u64>(5 * n), want = r.array<u64>(5 * n);
            if (r.bad) return 2;
            emul_sc_muladd(a.data(), b.data(), cc.data(), got.data(), n);
            rc = compare("muladd", rec, got, want, nullptr, nullptr);
        } else {
            const auto a = r.array<u64>(5 * n), want = r.array<u64>(5 * n);
            const auto wok = r.array<uint8_t>(n);
            if (r.bad || (op != 4 && (c < 1 || c > 64))) return 2;
            std::vector<uint8_t> gok(n);
            if (op == 4) emul_sc_invert(a.data(), got.data(), gok.data(), n);
            else emul_sc_invert_chunked(a.data(), got.data(), gok.data(), n, (int)c, op == 6);
            rc = compare("invert", rec, got, want, &gok, &wok);
        }
        if (rc) return rc;
        rows += n;
    }
    std::printf("scalar_ext_san: %zu rows match\n", rows);
    return 0;
}
