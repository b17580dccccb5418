// scvec_san.cpp -- TEST-ONLY stand-alone program: replays a vector file through the driver of the scalar vector ops
// (scvec_emul.cpp) and compares every output with the expected values the file carries.  Built with -fsanitize=address,undefined
// -fno-sanitize-recover=all by tests/test_scvec_emul.py and run as a child process: the exit status is the verdict (0: every row
// matched and no sanitizer report; 1: a mismatch; 2: a malformed file).
//
// The file is a sequence of records of little-endian 64-bit words: op 0 sum / 1 dot / 2 dot with a shared b / 3 powers (4: end),
// n, terms, then the inputs (a: n * terms * 5 words; b: as a, or terms * 5 words when shared; powers: x of n * 5 words), then the
// expected output (n * 5 words; powers: n * terms * 5).  Inputs and outputs sit in heap blocks of exactly their size: a record
// index past the row's end or an output row past n is a report.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <vector>
#include "scvec_emul.cpp"

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
        const uint64_t op = w[pos++];
        if (op == 4) break;
        if (op > 3 || w.size() - pos < 2) return 2;
        const size_t n = w[pos], terms = w[pos + 1];
        pos += 2;
        if (n > (1u << 12) || terms > (1u << 18) || n * terms > (1u << 19)) return 2;
        const size_t na = op == 3 ? n * 5 : n * terms * 5, nb = op == 1 ? n * terms * 5 : op == 2 ? terms * 5 : 0, nout = op == 3 ? n * terms * 5 : n * 5;
        if (w.size() - pos < na + nb + nout) return 2;
        const std::vector<uint64_t> a(w.begin() + pos, w.begin() + pos + na), b(w.begin() + pos + na, w.begin() + pos + na + nb);
        pos += na + nb;
        std::vector<uint64_t> out(nout);
        if (op == 0) emul_sc_sum_rows(a.data(), terms, out.data(), n);
        else if (op == 3) emul_sc_powers(a.data(), terms, out.data(), n);
        else emul_sc_dot_rows(a.data(), b.data(), terms, op == 2 ? 1u : 0u, out.data(), n);
        for (size_t i = 0; i < nout; i++)
            if (out[i] != w[pos + i]) {
                std::fprintf(stderr, "record %zu: row %zu: limb %zu differs from the file's\n", records, i / (nout / (n ? n : 1)), i % 5);
                return 1;
            }
        pos += nout;
        rows += n;
    }
    if (emul_scvec_bound_failures()) return 1;
    std::printf("scvec_san: %zu records, %zu rows match\n", records, rows);
    return 0;
}
