// Stand-alone driver of csrc/bam_span.h for tests/test_bam_span.py: built with -fsanitize=address,undefined, results on stdout.
//   bam_span_check <file>     the file holds whitespace-separated numbers:
//                             n_blocks, then file_off isize per block; n_voffs, then the virtual offsets; n_parts, then the part sizes
// Prints   lin_off ... / starts ... / n_chains k / len L        (SpanTables)
//          offsets ... / total T / staged <bytes>               (UploadParts: add, then stage into a buffer of exactly `total` bytes
//                                                                and read every part back through at<>)
#include <cstdio>
#include <cstdlib>
#include "bam_span.h"

int main(int argc, char** argv) {
    FILE* f = argc == 2 ? fopen(argv[1], "r") : nullptr;
    if (!f) { fprintf(stderr, "usage: bam_span_check <file>\n"); return 2; }
    auto next = [&]() -> size_t {
        unsigned long long v = 0;
        if (fscanf(f, "%llu", &v) != 1) { fprintf(stderr, "short input\n"); exit(2); }
        return size_t(v);
    };
    std::vector<cto_bgzf_block> blocks(next());
    for (auto& b : blocks) { b = cto_bgzf_block{}; b.file_off = next(); b.isize = uint32_t(next()); }
    std::vector<uint64_t> voffs(next());
    for (auto& v : voffs) v = next();
    std::vector<size_t> sizes(next());
    for (auto& s : sizes) s = next();
    fclose(f);

    cto::SpanTables t;
    t.lay_out(blocks.data(), int64_t(blocks.size()));
    t.map_starts(blocks.data(), int64_t(blocks.size()), voffs.data(), int64_t(voffs.size()));
    printf("lin_off");
    for (int64_t v : t.lin_off) printf(" %lld", (long long)v);
    printf("\nstarts");
    for (int64_t v : t.starts) printf(" %lld", (long long)v);
    printf("\nn_chains %d\nlen %lld\n", t.n_chains, (long long)t.len);

    cto::UploadParts parts;
    std::vector<std::vector<unsigned char>> src(sizes.size());
    for (size_t i = 0; i < sizes.size(); ++i) {
        src[i].assign(sizes[i], (unsigned char)(i + 1));
        parts.add(src[i].data(), sizes[i]);
    }
    printf("offsets");
    for (int i = 0; i < parts.n; ++i) printf(" %zu", parts.off[i]);
    printf("\ntotal %zu\n", parts.total);
    std::vector<char> pinned(parts.total, 0);
    parts.stage(pinned.data());
    size_t staged = 0;
    for (int i = 0; i < parts.n; ++i)
        for (size_t k = 0; k < parts.bytes[i]; ++k) staged += parts.at<unsigned char>(pinned.data(), i)[k] == (unsigned char)(i + 1);
    size_t nonzero = 0;
    for (char c : pinned) nonzero += c != 0;
    printf("staged %zu\n", staged == nonzero ? staged : size_t(-1));      // every byte of every part in its place, nothing anywhere else
    return 0;
}
