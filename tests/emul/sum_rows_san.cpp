// sum_rows_san.cpp -- TEST-ONLY stand-alone program: replays a vector file through the driver of the point sums
// (sum_rows_emul.cpp) and compares every output with the expected values the file carries.  Built with
// -fsanitize=address,undefined -fno-sanitize-recover=all by tests/test_sum_rows_emul.py and run as a child process: the exit
// status is the verdict (0: every row matched and no sanitizer report; 1: a mismatch; 2: a malformed file).
//
// The file is a sequence of records of little-endian 64-bit words: 1 (0: end), terms, n, n * terms * 20 words of points, n * 20
// words of expected sums, n * terms * 4 words of encodings, n * 4 words of expected encodings, n words of expected accept bits.
// Inputs and outputs sit in heap blocks of exactly their size: a record read past a row's end or a partial past the plan's
// count is a report.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <vector>
#include "sum_rows_emul.cpp"

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
        if (w[pos++] == 0) break;
        if (w.size() - pos < 2) return 2;
        const size_t terms = w[pos], n = w[pos + 1];
        pos += 2;
        if (terms > (1u << 20) || n > (1u << 20) || (w.size() - pos) / 24 < n * terms || w.size() - pos < 24 * n * terms + 25 * n) return 2;
        const std::vector<uint64_t> points(w.begin() + pos, w.begin() + pos + 20 * n * terms);
        pos += 20 * n * terms;
        const size_t want_pts = pos;
        pos += 20 * n;
        const std::vector<uint64_t> enc(w.begin() + pos, w.begin() + pos + 4 * n * terms);
        pos += 4 * n * terms;
        const size_t want_enc = pos, want_ok = pos + 4 * n;
        pos += 5 * n;
        std::vector<uint64_t> pts(20 * n), out(4 * n);
        std::vector<uint8_t> ok(n);
        emul_ed_sum_rows(points.data(), terms, pts.data(), n);
        emul_ris_sum_rows(reinterpret_cast<const uint8_t*>(enc.data()), terms, reinterpret_cast<uint8_t*>(out.data()), ok.data(), n);
        for (size_t i = 0; i < n; i++) {
            for (size_t k = 0; k < 20; k++)
                if (pts[20 * i + k] != w[want_pts + 20 * i + k]) {
                    std::fprintf(stderr, "record %zu: row %zu: limb %zu of the sum differs\n", records, i, k);
                    return 1;
                }
            for (size_t k = 0; k < 4; k++)
                if (out[4 * i + k] != w[want_enc + 4 * i + k]) {
                    std::fprintf(stderr, "record %zu: row %zu: the encoding differs in word %zu\n", records, i, k);
                    return 1;
                }
            if (ok[i] != w[want_ok + i]) {
                std::fprintf(stderr, "record %zu: row %zu: the accept bit differs\n", records, i);
                return 1;
            }
        }
        rows += n;
    }
    std::printf("sum_rows_san: %zu records, %zu rows match\n", records, rows);
    return 0;
}
