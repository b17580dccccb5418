// shared_scalar_plan_san.cpp -- TEST-ONLY stand-alone program: replays a vector file through the driver of zc_shared_scalar.h
// (shared_scalar_plan_emul.cpp) and compares every word with the expected values the file carries.  Built with
// -fsanitize=address,undefined -fno-sanitize-recover=all by tests/test_shared_scalar_plan_emul.py and run as a child process: the
// exit status is the verdict (0: every case matched and no sanitizer report; 1: a mismatch; 2: a malformed file).
//
// The file is a sequence of records of little-endian 64-bit words: 1 (0: end), the five words of the scalar, then the
// emul_shared_plan_words() expected words.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <vector>
#include "shared_scalar_plan_emul.cpp"

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) return 2;
    const std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (raw.size() % 8) return 2;
    std::vector<int64_t> w(raw.size() / 8);
    std::copy(raw.begin(), raw.end(), reinterpret_cast<char*>(w.data()));
    const size_t nw = (size_t)emul_shared_plan_words();
    size_t pos = 0, cases = 0;
    for (;; cases++) {
        if (pos >= w.size()) return 2;
        const int64_t more = w[pos++];
        if (more == 0) break;
        if (more != 1 || w.size() - pos < 5 + nw) return 2;
        // exactly the scalar and exactly the words the driver writes, each in a heap block of its own
        const std::vector<uint64_t> k(w.begin() + pos, w.begin() + pos + 5);
        std::vector<int64_t> got(nw, -1);
        emul_shared_plan(k.data(), got.data());
        for (size_t i = 0; i < nw; i++)
            if (got[i] != w[pos + 5 + i]) {
                std::fprintf(stderr, "case %zu: word %zu: got %lld, want %lld\n", cases, i, (long long)got[i], (long long)w[pos + 5 + i]);
                return 1;
            }
        pos += 5 + nw;
    }
    std::printf("shared_scalar_plan_san: %zu cases match\n", cases);
    return 0;
}
