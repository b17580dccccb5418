// shared_lincomb_plan_san.cpp -- TEST-ONLY stand-alone program: replays a vector file through the driver of the joint schedule
// (shared_lincomb_plan_emul.cpp) and compares every word with the expected values the file carries.  Built with
// -fsanitize=address,undefined -fno-sanitize-recover=all by tests/test_shared_lincomb_plan_emul.py and run as a child process:
// the exit status is the verdict (0: every case matched and no sanitizer report; 1: a mismatch; 2: a malformed file).
//
// The file is a sequence of records of little-endian 64-bit words: the term count 1..8 (0: end), terms * 5 words of scalars,
// then the emul_shared_lincomb_plan_words() expected words.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <vector>
#include "shared_lincomb_plan_emul.cpp"

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) return 2;
    const std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (raw.size() % 8) return 2;
    std::vector<int64_t> w(raw.size() / 8);
    std::copy(raw.begin(), raw.end(), reinterpret_cast<char*>(w.data()));
    const size_t nw = (size_t)emul_shared_lincomb_plan_words();
    size_t pos = 0, cases = 0;
    for (;; cases++) {
        if (pos >= w.size()) return 2;
        const int64_t terms = w[pos++];
        if (terms == 0) break;
        if (terms < 1 || terms > zc::SHARED_LINCOMB_MAX_TERMS || w.size() - pos < 5 * (size_t)terms + nw) return 2;
        // exactly the scalars and exactly the words the driver writes, each in a heap block of its own
        const std::vector<uint64_t> k(w.begin() + pos, w.begin() + pos + 5 * terms);
        std::vector<int64_t> got(nw, -1);
        emul_shared_lincomb_plan(k.data(), (size_t)terms, got.data());
        for (size_t i = 0; i < nw; i++)
            if (got[i] != w[pos + 5 * terms + i]) {
                std::fprintf(stderr, "case %zu: word %zu: got %lld, want %lld\n", cases, i, (long long)got[i], (long long)w[pos + 5 * terms + i]);
                return 1;
            }
        pos += 5 * terms + nw;
    }
    std::printf("shared_lincomb_plan_san: %zu cases match\n", cases);
    return 0;
}
