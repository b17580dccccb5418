// fe_muld_san.cpp -- TEST-ONLY stand-alone program: replays a vector file through the host build of fp_mul_d and of the addition
// formulas that call it (fe_muld_emul.cpp) and compares every output word with the expected values the file carries.  Built with
// -fsanitize=address,undefined -fno-sanitize-recover=all by tests/test_fe_muld_emul.py and run as a child process: the exit
// status is the verdict (0: every row matched and no sanitizer report; 1: a mismatch; 2: a malformed file).
//
// The file is a sequence of records of little-endian words: op, n (64-bit each), then for op 1 n x 9 32-bit register limbs and
// n x 5 expected 64-bit limbs of fe_store_canon(fp_mul_d(x)); for op 2 + form (form 0..5 of emul_muld_ed_add) n x 20 words of p,
// of q and of the expected p + q; op 0: end.  Inputs and outputs live in heap blocks of exactly their size.
#include <fstream>
#include <iterator>
#include <vector>
#include "fe_muld_emul.cpp"

namespace {
struct Reader {
    std::vector<uint8_t> buf;
    size_t pos = 0;
    bool bad = false;
    template <class T>
    std::vector<T> array(size_t count)
    {
        std::vector<T> v(count);
        if (count * sizeof(T) > buf.size() - pos) {
            bad = true;
            return v;
        }
        if (count) std::memcpy(v.data(), buf.data() + pos, count * sizeof(T));
        pos += count * sizeof(T);
        return v;
    }
};
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
        const auto head = r.array<u64>(2);
        const u64 op = head[0], n = head[1];
        if (r.bad || op > 7 || n > (1u << 20)) return 2;
        if (op == 0) break;
        std::vector<u64> got, want;
        size_t per_row;
        if (op == 1) {
            const auto x = r.array<u32>(9 * n);
            want = r.array<u64>(5 * n);
            if (r.bad) return 2;
            std::vector<u32> raw(9 * n);
            std::vector<u64> ref(5 * n);
            got.assign(5 * n, 0xA5A5A5A5A5A5A5A5ull);
            emul_fe_muld(x.data(), raw.data(), got.data(), ref.data(), n);
            if (ref != got) {
                std::fprintf(stderr, "record %llu: fp_mul_d and mont_mul(D_M, .) differ\n", (unsigned long long)rec);
                return 1;
            }
            per_row = 5;
        } else {
            const auto p = r.array<u64>(20 * n), q = r.array<u64>(20 * n);
            want = r.array<u64>(20 * n);
            if (r.bad) return 2;
            got.assign(20 * n, 0xA5A5A5A5A5A5A5A5ull);
            emul_muld_ed_add(p.data(), q.data(), got.data(), n, (int)op - 2);
            per_row = 20;
        }
        for (size_t i = 0; i < want.size(); i++)
            if (got[i] != want[i]) {
                std::fprintf(stderr, "record %llu: row %zu word %zu: got %llx, want %llx\n", (unsigned long long)rec, i / per_row, i % per_row,
                             (unsigned long long)got[i], (unsigned long long)want[i]);
                return 1;
            }
        rows += n;
    }
    std::printf("fe_muld_san: %zu rows match\n", rows);
    return 0;
}
