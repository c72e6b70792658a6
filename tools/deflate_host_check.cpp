// Stand-alone check of the host BGZF coder (clairs_to_amd/csrc/deflate_host.h) for a sanitizer build:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/deflate_host_check.cpp -lz -o deflate_host_check
// Every shape of tests/test_bgzf_deflate.py is coded block by block and inflated again with zlib; exit status 0 = all equal.
#include <zlib.h>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../clairs_to_amd/csrc/deflate_host.h"

using Bytes = std::vector<uint8_t>;
namespace df = cto::dfl;

static uint32_t rng_state = 12345;
static uint32_t rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

static int check(const char* name, const Bytes& in) {
    int bad = 0;
    size_t n_blocks = 0, out_bytes = 0;
    int types[3] = {0, 0, 0};
    for (size_t at = 0; at < in.size(); at += df::kPayload, ++n_blocks) {
        const int n = int(std::min<size_t>(df::kPayload, in.size() - at));
        Bytes out(df::kSlot);
        df::BlockInfo info;
        const int size = df::encode_block(in.data() + at, n, out.data(), &info);
        ++types[info.type];
        out_bytes += size_t(size);
        if (size > n + 31 || size != 1 + (out[16] | (out[17] << 8))) { printf("%s: block %zu: size %d, n %d\n", name, n_blocks, size, n); ++bad; }
        if ((info.bits[info.type] + 7) / 8 != size - 26) { printf("%s: block %zu: payload is not ceil(bits / 8)\n", name, n_blocks); ++bad; }
        Bytes back(size_t(n) + 1);
        z_stream zs;
        memset(&zs, 0, sizeof zs);
        inflateInit2(&zs, -15);
        zs.next_in = out.data() + 18;
        zs.avail_in = uInt(size - 26);
        zs.next_out = back.data();
        zs.avail_out = uInt(back.size());
        const int rc = inflate(&zs, Z_FINISH);
        const bool same = rc == Z_STREAM_END && zs.total_out == uLong(n) && zs.avail_in == 0 && !memcmp(back.data(), in.data() + at, size_t(n));
        inflateEnd(&zs);
        if (!same) { printf("%s: block %zu does not inflate to its input (zlib %d)\n", name, n_blocks, rc); ++bad; }
        const uint8_t* t = out.data() + size - 8;
        const uint32_t crc = t[0] | (t[1] << 8) | (t[2] << 16) | (uint32_t(t[3]) << 24), isize = t[4] | (t[5] << 8) | (t[6] << 16) | (uint32_t(t[7]) << 24);
        if (crc != uint32_t(crc32(crc32(0L, Z_NULL, 0), in.data() + at, uInt(n))) || isize != uint32_t(n)) { printf("%s: block %zu: trailer\n", name, n_blocks); ++bad; }
    }
    printf("%-12s %8zu -> %8zu bytes, %zu blocks (stored %d, fixed %d, dynamic %d)%s\n", name, in.size(), out_bytes, n_blocks, types[0], types[1], types[2],
           bad ? "  FAILED" : "");
    return bad;
}

int main() {
    int bad = 0;
    {   // no bytes: the 28 bytes of BGZF's end block
        const uint8_t eof[28] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0, 27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        Bytes out(df::kSlot);
        if (df::encode_block(nullptr, 0, out.data()) != 28 || memcmp(out.data(), eof, 28)) { printf("empty block: not the end block\n"); ++bad; }
    }
    for (size_t n : {size_t(1), size_t(2), size_t(3), size_t(4), size_t(0xff00 - 1), size_t(0xff00), size_t(0xff00 + 1), size_t(2 * 0xff00 + 7)}) {
        Bytes b(n);
        for (size_t i = 0; i < n; ++i) b[i] = uint8_t("ACGTNacgtn!#"[rng() % 12]);
        bad += check(("text " + std::to_string(n)).c_str(), b);
    }
    bad += check("equal", Bytes(0xff00, 'I'));
    { Bytes b(0xff00); for (size_t i = 0; i < b.size(); ++i) b[i] = uint8_t("ab"[i % 2]); bad += check("period 2", b); }
    { Bytes b(0xff00); for (size_t i = 0; i < b.size(); ++i) b[i] = uint8_t("abc"[i % 3]); bad += check("period 3", b); }
    { Bytes b(0xff00); for (auto& x : b) x = uint8_t(rng() >> 11); bad += check("random", b); }
    { Bytes b(40000); for (size_t i = 0; i < b.size(); ++i) b[i] = uint8_t(i % 7 ? (i * i) >> 5 : i); bad += check("all bytes", b); }
    {   // repeats at every distance class and of every length
        Bytes b;
        for (int len = 3; len <= 258; ++len) {
            const size_t from = b.size();
            for (int i = 0; i < len; ++i) b.push_back(uint8_t(rng() >> 9));
            b.push_back(uint8_t(len));
            b.insert(b.end(), b.begin() + long(from), b.begin() + long(from) + len);
        }
        b.resize(0xff00);
        bad += check("lengths", b);
    }
    { Bytes b(32769 + 64); for (auto& x : b) x = uint8_t(rng() >> 7); memcpy(b.data() + 32769, b.data(), 64); bad += check("far", b); }
    { Bytes b(700); for (size_t i = 0; i < b.size(); ++i) b[i] = uint8_t(i * 37 + (i >> 3)); bad += check("no match", b); }
    printf(bad ? "FAILED: %d\n" : "all shapes round-trip\n", bad);
    return bad ? 1 : 0;
}
