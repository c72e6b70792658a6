// The size the host BGZF coder (clairs_to_amd/csrc/deflate_host.h) gives for a file's bytes, for tools/deflate_bench.py --variants:
// built once per candidate with -DCTO_DEFLATE_SEG=... and -DCTO_DEFLATE_PROBES=..., so that the segment length and the probe set can be
// chosen by what they cost in bytes.  Prints: in_bytes out_bytes blocks stored fixed dynamic.
#include <cstdio>
#include <vector>
#include "../clairs_to_amd/csrc/deflate_host.h"

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: deflate_ratio FILE\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint8_t> in;
    uint8_t buf[1 << 16];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) in.insert(in.end(), buf, buf + n);
    fclose(f);
    namespace df = cto::dfl;
    std::vector<uint8_t> out(df::kSlot);
    long long total = 0, blocks = 0, types[3] = {0, 0, 0};
    for (size_t at = 0; at < in.size(); at += df::kPayload, ++blocks) {
        df::BlockInfo info;
        total += df::encode_block(in.data() + at, int(std::min<size_t>(df::kPayload, in.size() - at)), out.data(), &info);
        ++types[info.type];
    }
    printf("%zu %lld %lld %lld %lld %lld\n", in.size(), total, blocks, types[0], types[1], types[2]);
    return 0;
}
