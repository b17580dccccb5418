// gens_san.cpp -- TEST-ONLY stand-alone program: replays a vector file through the driver of the generator sets (gens_emul.cpp)
// and compares every output with the expected values the file carries.  Built with -fsanitize=address,undefined
// -fno-sanitize-recover=all by tests/test_gens_emul.py and run as a child process: the exit status is the verdict (0: every row
// matched and no sanitizer report; 1: a mismatch; 2: a malformed file).
//
// The file is a sequence of records of little-endian 64-bit words: count 1..8 (0: end), n, count * 20 words of points, n * count
// * 5 words of scalars, n * 4 words of expected encodings.  The tables of a record sit in a heap block of exactly
// 33 * 128 * 128 * count bytes, scalars and outputs in blocks of exactly their size: an index past a term's table, past the
// last term or past digit 32 is a report.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <vector>
#include "gens_emul.cpp"

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) return 2;
    const std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (raw.size() % 8) return 2;
    std::vector<uint64_t> w(raw.size() / 8);
    std::copy(raw.begin(), raw.end(), reinterpret_cast<char*>(w.data()));
    size_t pos = 0, records = 0, rows = 0;
    for (;; records++) {
        if (pos >= w.size()) return 2;
        const size_t count = w[pos++];
        if (count == 0) break;
        if (count > (size_t)zc::GENS_MAX || pos >= w.size()) return 2;
        const size_t n = w[pos++];
        if (n > (1u << 20) || w.size() - pos < 20 * count + 5 * count * n + 4 * n) return 2;
        const std::vector<uint64_t> points(w.begin() + pos, w.begin() + pos + 20 * count);
        pos += 20 * count;
        const std::vector<uint64_t> k(w.begin() + pos, w.begin() + pos + 5 * count * n);
        pos += 5 * count * n;
        static_assert(sizeof(zc::u32) * zc::GENS_TABLE_WORDS == 33 * 128 * 128, "one generator's table");
        zc::u32* const tables = static_cast<zc::u32*>(std::malloc(33 * 128 * 128 * count));
        if (!tables) return 2;
        int rc = emul_gens_build(points.data(), count, tables) == -1 ? 0 : 1;
        std::vector<uint64_t> pts(20 * n), enc(4 * n);
        if (!rc) {
            emul_ed_mul_gens(tables, count, k.data(), pts.data(), n);
            emul_ris_mul_gens_compress(tables, count, k.data(), reinterpret_cast<uint8_t*>(enc.data()), n);
        }
        std::free(tables);
        if (rc) {
            std::fprintf(stderr, "record %zu: a generator was refused\n", records);
            return 1;
        }
        for (size_t i = 0; i < 4 * n; i++)
            if (enc[i] != w[pos + i]) {
                std::fprintf(stderr, "record %zu: row %zu: word %zu of the encoding differs\n", records, i / 4, i % 4);
                return 1;
            }
        for (size_t i = 0; i < 20 * n; i++)
            if (pts[i] >> 52) {
                std::fprintf(stderr, "record %zu: row %zu: a limb above 2^52\n", records, i / 20);
                return 1;
            }
        pos += 4 * n;
        rows += n;
    }
    std::printf("gens_san: %zu records, %zu rows match\n", records, rows);
    return 0;
}
