// ris_dac_san.cpp -- TEST-ONLY stand-alone program: replays a vector file through the host build of the device functions
// behind zc_ris_double_and_compress (ris_dac_emul.cpp) and compares every output byte with the expected encodings the file
// carries.  Built with -fsanitize=address,undefined -fno-sanitize-recover=all by tests/test_ris_dac_emul.py and run as a child
// process: the exit status is the verdict (0: every row matched and no sanitizer report; 1: a mismatch; 2: a malformed file).
//
// The file is a sequence of records of little-endian 64-bit words: op, n, c, then n x 20 words of points and n x 32 expected
// bytes.  op 1: one row per lane, 2 / 3: shared inversions with chunk c on the column-ordered / independent-chain
// multiplier, 0: end.  Inputs and outputs live in heap blocks of exactly their size, so an access outside the rows is a report.
#include <fstream>
#include <iterator>
#include <vector>
#include "ris_dac_emul.cpp"

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
        if (r.bad || op > 3 || n > (1u << 20)) return 2;
        if (op == 0) break;
        const auto p = r.array<u64>(20 * n);
        const auto want = r.array<uint8_t>(32 * n);
        if (r.bad || (op != 1 && (c < 1 || c > 64))) return 2;
        std::vector<uint8_t> got(32 * n, 0xA5);
        if (op == 1) emul_ris_dac_rows(p.data(), got.data(), n);
        else emul_ris_dac_chunked(p.data(), got.data(), n, (int)c, op == 3);
        for (size_t i = 0; i < want.size(); i++)
            if (got[i] != want[i]) {
                std::fprintf(stderr, "record %llu: row %zu byte %zu: got %02x, want %02x\n", (unsigned long long)rec, i / 32, i % 32, got[i], want[i]);
                return 1;
            }
        rows += n;
    }
    std::printf("ris_dac_san: %zu rows match\n", rows);
    return 0;
}
