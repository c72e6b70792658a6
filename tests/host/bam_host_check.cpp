// Stand-alone driver of csrc/bam_host.h for tests/test_bam_host.py: built with -fsanitize=address,undefined, results on stdout.
//   bam_host_check <bam> <ctg> <start> <end> [<bai>]    start / end 1-based inclusive; the index is <bam>.bai unless named
//       one line per record the region reader yields that is not wholly in front of the region, no filter applied:
//           pos flag mapq l_seq CIGAR rlen qlen enters [HP]
//       CIGAR = the effective operations (`*` for none), enters = BamRegion::enters, HP = the value of each integer HP field
//   bam_host_check tbi <inflated index> <ctg>
//       `found 0|1`, then `beg end` per chunk of the contig
// An error prints `error: <text>` on stdout and ends with status 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "bam_host.h"

static int fail(const std::string& what) {
    printf("error: %s\n", what.c_str());
    return 1;
}

int main(int argc, char** argv) {
    if (argc == 4 && strcmp(argv[1], "tbi") == 0) {
        std::vector<uint8_t> idx;
        std::vector<cto::Chunk> chunks;
        std::string err;
        bool found = false;
        if (!cto::read_index_file(argv[2], &idx, &err)) return fail(err);
        if (!cto::tbi_contig_chunks(idx.data(), idx.size(), argv[3], &chunks, &found, &err)) return fail(err);
        printf("found %d\n", int(found));
        for (const cto::Chunk& c : chunks) printf("%llu %llu\n", (unsigned long long)c.beg, (unsigned long long)c.end);
        return 0;
    }
    if (argc != 5 && argc != 6) { fprintf(stderr, "usage: bam_host_check <bam> <ctg> <start> <end> [<bai>] | tbi <index> <ctg>\n"); return 2; }
    cto::BamRegion rg;
    if (!rg.open("check", argv[1], argc == 6 ? argv[5] : nullptr, argv[2], atoll(argv[3]) - 1, atoll(argv[4]), false, false)) return fail(rg.err);
    cto::BamRecord b;
    for (int got; (got = rg.next(&b)) != 0;) {
        if (got < 0 || !rg.lay_out(&b)) return fail(rg.err);
        const int enters = rg.enters(b);
        if (enters < 0) return fail(rg.err);
        if (int64_t(b.pos) + std::max<int64_t>(b.rlen, 1) <= rg.beg0) continue;
        printf("%d %d %d %d ", b.pos, b.flag, b.mapq, b.l_seq);
        if (b.n_ops == 0) printf("*");
        for (int i = 0; i < b.n_ops; ++i) printf("%u%c", b.op(i) >> 4, "MIDNSHP=X???????"[b.op(i) & 15]);
        printf(" %lld %lld %d", (long long)b.rlen, (long long)b.qlen, enters);
        const uint8_t* aux = b.aux;
        long long val;
        for (cto::AuxField f; cto::aux_next(&aux, b.end, &f);)
            if (f.t0 == 'H' && f.t1 == 'P' && cto::aux_int(f, &val)) printf(" %lld", val);
        printf("\n");
    }
    return 0;
}
