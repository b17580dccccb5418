// hash_san.cpp -- TEST-ONLY stand-alone program: replays a vector file through the host build of the SHA-512 rows
// (hash_emul.cpp) and compares every row with the expected values the file carries.  Built with
// -fsanitize=address,undefined -fno-sanitize-recover=all by tests/test_hash_emul.py and run as a child process: the exit status
// is the verdict (0: every row matched and no sanitizer report; 1: a mismatch; 2: a malformed file).
//
// The file is a sequence of records of little-endian 64-bit words: op + 1 (1: digests, 2: scalars, 3: points; 0: end), n,
// force_bytes, offset (the parts start that many bytes past an 8-byte boundary), prefix_len, nparts, nparts lengths, then the
// prefix, every part (n x part_len bytes) and the expected output (n x 64 / 40 / 160 bytes), each padded to a multiple of 8 bytes.
#include <fstream>
#include <iterator>
#include <vector>
#include "hash_emul.cpp"

namespace {
struct Reader {
    std::vector<uint8_t> buf;
    size_t pos = 0;
    bool bad = false;
    const uint8_t* take(size_t bytes)
    {
        const size_t padded = (bytes + 7) & ~(size_t)7;
        if (padded > buf.size() - pos) {
            bad = true;
            return nullptr;
        }
        const uint8_t* p = buf.data() + pos;
        pos += padded;
        return p;
    }
    u64 word()
    {
        const uint8_t* p = take(8);
        u64 w = 0;
        if (p) std::memcpy(&w, p, 8);
        return w;
    }
    // a copy of exactly `bytes` bytes that starts `offset` bytes into a heap block of its own and ends with the block, so
    // that a read past the end is an AddressSanitizer report.  (operator new aligns to 16: offset is the address mod 8)
    std::vector<uint8_t> bytes_at(size_t bytes, size_t offset)
    {
        std::vector<uint8_t> v(offset + bytes);
        const uint8_t* p = take(bytes);
        if (p && bytes) std::memcpy(v.data() + offset, p, bytes);
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
        const u64 op1 = r.word();
        if (r.bad || op1 > 3) return 2;
        if (op1 == 0) break;
        const u64 n = r.word(), force = r.word(), offset = r.word(), prefix_len = r.word(), nparts = r.word();
        if (r.bad || n > (1u << 16) || offset > 7 || prefix_len > 256 || nparts < 1 || nparts > 4) return 2;
        size_t lens[4] = {0, 0, 0, 0};
        for (u64 j = 0; j < nparts; j++) lens[j] = (size_t)r.word();
        for (u64 j = 0; j < nparts; j++)
            if (r.bad || lens[j] < 1 || lens[j] > 65535) return 2;
        const std::vector<uint8_t> prefix = r.bytes_at(prefix_len, 0);
        std::vector<uint8_t> parts[4];
        const uint8_t* ptrs[4] = {nullptr, nullptr, nullptr, nullptr};
        for (u64 j = 0; j < nparts; j++) {
            parts[j] = r.bytes_at(n * lens[j], offset);
            ptrs[j] = parts[j].data() + offset;
        }
        const size_t out_bytes = op1 == 1 ? 64 : op1 == 2 ? 40 : 160;
        const std::vector<uint8_t> want = r.bytes_at(n * out_bytes, 0);
        if (r.bad) return 2;
        std::vector<u64> got((n * out_bytes + 7) / 8);                      // 8-byte aligned for the limb outputs, exactly n rows
        if (emul_hash_rows((int)op1 - 1, prefix.data(), prefix_len, ptrs, lens, nparts, got.data(), n, (int)force) < 0) return 2;
        const uint8_t* g = reinterpret_cast<const uint8_t*>(got.data());
        for (size_t i = 0; i < n * out_bytes; i++)
            if (g[i] != want[i]) {
                std::fprintf(stderr, "record %llu (op %llu): row %zu byte %zu: got %02x, want %02x\n", (unsigned long long)rec, (unsigned long long)(op1 - 1),
                             i / out_bytes, i % out_bytes, g[i], want[i]);
                return 1;
            }
        rows += n;
    }
    std::printf("hash_san: %zu rows match\n", rows);
    return 0;
}
