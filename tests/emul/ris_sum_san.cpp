// ris_sum_san.cpp -- TEST-ONLY stand-alone program: replays a vector file through the host build of the device functions
// behind zc_ris_lincomb_sum (ris_sum_emul.cpp) -- the prepare pass, the rows pass and the reduction of the base term, in the
// product's order -- and compares the records, the scalars and the accept mask with the expected values the file carries.
// Built with -fsanitize=address,undefined -fno-sanitize-recover=all by tests/test_ris_lincomb_sum_emul.py and run as a child
// process: the exit status is the verdict (0: everything matched and no sanitizer report; 1: a mismatch; 2: a malformed file).
//
// The file is a sequence of records of little-endian 64-bit words: op (1; 0 ends the file), n, terms, flags (bit 0: base
// scalars, bit 1: weights), then n x terms x 32 bytes of encodings, n x terms x 5 words of scalars, n x 5 words of base
// scalars and of weights when present, and the expected (n terms + base) x 20 words of records, as many x 5 words of scalars
// and n bytes of mask.  Inputs, workspace and outputs live in heap blocks of exactly their size, so an access outside the rows
// is a report.
#include <fstream>
#include <iterator>
#include <vector>
#include "ris_sum_emul.cpp"

namespace {
struct Reader {
    std::vector<uint8_t> buf;
    size_t pos = 0;
    bool bad = false;
    const uint8_t* take(size_t bytes)
    {
        if (bytes > buf.size() - pos) {
            bad = true;
            return nullptr;
        }
        const uint8_t* p = buf.data() + pos;
        pos += bytes;
        return p;
    }
    u64 word()
    {
        const uint8_t* p = take(8);
        u64 w = 0;
        if (p) std::memcpy(&w, p, 8);
        return w;
    }
    template <class T>
    std::vector<T> array(size_t count)
    {
        std::vector<T> v(count);
        const uint8_t* p = take(count * sizeof(T));
        if (p && count) std::memcpy(v.data(), p, count * sizeof(T));
        return v;
    }
};
template <class T>
bool same(const char* what, u64 rec, const std::vector<T>& got, const std::vector<T>& want, size_t per_row)
{
    for (size_t i = 0; i < want.size(); i++)
        if (got[i] != want[i]) {
            std::fprintf(stderr, "record %llu: %s: row %zu element %zu: got %llx, want %llx\n", (unsigned long long)rec, what, i / per_row, i % per_row,
                         (unsigned long long)got[i], (unsigned long long)want[i]);
            return false;
        }
    return true;
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
        const u64 op = r.word(), n = r.word(), terms = r.word(), flags = r.word();
        if (r.bad || op > 1 || n > (1u << 16) || terms > 64 || flags > 3) return 2;
        if (op == 0) break;
        if (n == 0 || terms == 0) return 2;
        const bool base = flags & 1, weighted = flags & 2;
        const size_t pairs = n * terms, count = pairs + (base ? 1 : 0);
        const auto in32 = r.array<u64>(4 * pairs);                                  // as words: 8-byte aligned, as the kernel requires
        const auto k = r.array<u64>(5 * pairs);
        const auto kb = r.array<u64>(base ? 5 * n : 0);
        const auto z = r.array<u64>(weighted ? 5 * n : 0);
        const auto want_p = r.array<u64>(20 * count);
        const auto want_s = r.array<u64>(5 * count);
        const auto want_ok = r.array<uint8_t>(n);
        if (r.bad) return 2;
        std::vector<u64> points(20 * count, 0xA5A5A5A5A5A5A5A5ull), scalars(5 * count, 0xA5A5A5A5A5A5A5A5ull), t(base ? 5 * n : 0);
        std::vector<uint8_t> term_flags(pairs, 0xA5), ok(n, 0xA5);
        emul_ris_sum_prepare(reinterpret_cast<const uint8_t*>(in32.data()), k.data(), weighted ? z.data() : nullptr, points.data(), scalars.data(), term_flags.data(),
                             terms, pairs);
        emul_ris_sum_rows(term_flags.data(), scalars.data(), base ? kb.data() : nullptr, weighted ? z.data() : nullptr, ok.data(), base ? t.data() : nullptr,
                          base ? points.data() + 20 * pairs : nullptr, terms, n);
        if (base) emul_sc_sum(t.data(), n, scalars.data() + 5 * pairs, 64, 4, 3);
        if (!same("points", rec, points, want_p, 20) || !same("scalars", rec, scalars, want_s, 5) || !same("ok", rec, ok, want_ok, 1)) return 1;
        rows += n;
    }
    std::printf("ris_sum_san: %zu rows match\n", rows);
    return 0;
}
