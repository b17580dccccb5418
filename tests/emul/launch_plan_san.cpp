// launch_plan_san.cpp -- TEST-ONLY stand-alone program: replays a vector file through the driver of zc_launch_plan.h
// (launch_plan_emul.cpp) and compares every field with the expected values the file carries.  Built with
// -fsanitize=address,undefined -fno-sanitize-recover=all by tests/test_launch_plan_emul.py and run as a child process: the exit
// status is the verdict (0: every case matched and no sanitizer report; 1: a mismatch; 2: a malformed file).
//
// The file is a sequence of records of little-endian 64-bit words: kind + 1 (0: end), the number of arguments, the number of
// fields, the arguments, the expected fields.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <vector>
#include "launch_plan_emul.cpp"

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) return 2;
    const std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (raw.size() % 8) return 2;
    std::vector<int64_t> w(raw.size() / 8);
    std::copy(raw.begin(), raw.end(), reinterpret_cast<char*>(w.data()));
    size_t pos = 0, cases = 0;
    for (;; cases++) {
        if (pos >= w.size()) return 2;
        const int64_t kind1 = w[pos++];
        if (kind1 == 0) break;
        if (w.size() - pos < 2) return 2;
        const int64_t na = w[pos], nf = w[pos + 1];
        pos += 2;
        if (kind1 < 0 || na < 0 || na > 16 || nf < 1 || nf > 8 || (size_t)(na + nf) > w.size() - pos) return 2;
        // exactly the arguments and exactly eight fields, each in a heap block of its own: a read or write past either is a report
        const std::vector<int64_t> args(w.begin() + pos, w.begin() + pos + na);
        std::vector<int64_t> got(8, 0);
        if (emul_launch_plan((int)kind1 - 1, args.data(), (int)na, got.data()) != nf) return 2;
        for (int64_t i = 0; i < nf; i++)
            if (got[i] != w[pos + na + i]) {
                std::fprintf(stderr, "case %zu (kind %d): field %d: got %lld, want %lld\n", cases, (int)kind1 - 1, (int)i, (long long)got[i], (long long)w[pos + na + i]);
                return 1;
            }
        pos += na + nf;
    }
    std::printf("launch_plan_san: %zu cases match\n", cases);
    return 0;
}
