// dlog_san.cpp -- TEST-ONLY stand-alone program: replays a vector file through the driver of the bounded discrete logs
// (dlog_emul.cpp) and compares every output with the expected values the file carries.  Built with -fsanitize=address,undefined
// -fno-sanitize-recover=all by tests/test_dlog_emul.py and run as a child process: the exit status is the verdict (0: every row
// matched and no sanitizer report; 1: a mismatch; 2: a malformed file).
//
// The file is a sequence of records of little-endian 64-bit words: wire 0 / 1 (2: end), table_bits, flags, bound, n, 20 words of
// the generator, n * (20 or 4) words of rows, n words of expected m, n words of expected found, n words of expected ok.  Setup
// block, records, slots, rows and outputs sit in heap blocks of exactly their size: a slot index past 2^(t+1), a record index
// past 2^t or an output row past n is a report.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <vector>
#include "dlog_emul.cpp"

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
        const uint64_t wire = w[pos++];
        if (wire == 2) break;
        if (wire > 1 || w.size() - pos < 4 + 20) return 2;
        const unsigned t = (unsigned)w[pos], flags = (unsigned)w[pos + 1];
        const uint64_t bound = w[pos + 2];
        const size_t n = w[pos + 3];
        pos += 4;
        const size_t width = wire ? 4 : 20;
        if (!zc::dlog_bits_ok(t) || t > 10 || !zc::dlog_bound_ok(bound, t) || n > (1u << 16) || w.size() - pos < 20 + n * (width + 3)) return 2;
        const std::vector<uint64_t> point(w.begin() + pos, w.begin() + pos + 20);
        pos += 20;
        const std::vector<uint64_t> in(w.begin() + pos, w.begin() + pos + n * width);
        pos += n * width;
        std::vector<zc::u32> setup(zc::DLOG_SETUP_WORDS);
        if (emul_dlog_setup(point.data(), t, flags, setup.data()) != zc::DLOG_SETUP_OK) {
            std::fprintf(stderr, "record %zu: the generator was refused\n", records);
            return 1;
        }
        std::vector<uint64_t> recs(4 * zc::dlog_records(t)), slots(zc::dlog_slots(t)), m(n);
        std::vector<uint8_t> found(n), ok(n);
        emul_dlog_records(setup.data(), t, recs.data());
        if (emul_dlog_slots(recs.data(), t, slots.data()) != -1) {
            std::fprintf(stderr, "record %zu: a table entry occurs twice\n", records);
            return 1;
        }
        emul_dlog((int)wire, in.data(), n, setup.data(), recs.data(), slots.data(), t, flags, bound, m.data(), found.data(), ok.data());
        for (size_t i = 0; i < n; i++)
            if (m[i] != w[pos + i] || found[i] != w[pos + n + i] || ok[i] != w[pos + 2 * n + i]) {
                std::fprintf(stderr, "record %zu: row %zu: m %llu found %d ok %d differ from the file's\n", records, i, (unsigned long long)m[i], found[i], ok[i]);
                return 1;
            }
        pos += 3 * n;
        rows += n;
    }
    std::printf("dlog_san: %zu records, %zu rows match\n", records, rows);
    return 0;
}
