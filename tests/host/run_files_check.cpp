// Stand-alone driver of csrc/run_files.h for tests/test_run_files.py: one command per run, results on stdout, built with
// -fsanitize=address,undefined.  An error the code under test reports is a result ("error: <message>", exit 0), not a failure.
//   region <fasta> <ctg> <start> <end>    the bases, one line
//   bed <bed> <ctg>                       "b e" per merged interval
//   indel_regions <bed>                   "ctg b e" per merged interval, contigs in map order
//   map <path> [sniff]                    "<bytes> <FNV-1a 64 of them>"
//   spawn <argv...>                       the same of the child's stdout
#include "run_files.h"

using namespace cto::run_files;

static void print_bytes(const char* p, size_t n) {
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ (unsigned char)p[i]) * 1099511628211ull;
    printf("%zu %016llx\n", n, h);
}

int main(int argc, char** argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    std::string err;
    bool ok = false;
    if (cmd == "region" && argc == 6) {
        Mapped fa;
        FaiRec rec;
        std::string seq;
        ok = fa.open(argv[2], &err) && fai_lookup(argv[2], argv[3], &rec, &err) && read_region(fa, rec, atoll(argv[4]), atoll(argv[5]), &seq, &err);
        if (ok) printf("%s\n", seq.c_str());
    } else if (cmd == "bed" && argc == 4) {
        Mapped bed;
        std::vector<int64_t> iv;
        if ((ok = bed.open(argv[2], &err))) bed_intervals(bed.p ? bed.p : "", bed.n, argv[3], &iv);
        for (size_t i = 0; i + 1 < iv.size(); i += 2) printf("%lld %lld\n", (long long)iv[i], (long long)iv[i + 1]);
    } else if (cmd == "indel_regions" && argc == 3) {
        std::map<std::string, std::vector<int64_t>> by_ctg;
        ok = load_indel_regions(argv[2], &by_ctg, &err);
        if (ok)
            for (const auto& kv : by_ctg)
                for (size_t i = 0; i + 1 < kv.second.size(); i += 2) printf("%s %lld %lld\n", kv.first.c_str(), (long long)kv.second[i], (long long)kv.second[i + 1]);
    } else if (cmd == "map" && (argc == 3 || argc == 4)) {
        Mapped m;
        if ((ok = m.open(argv[2], &err, argc == 4))) print_bytes(m.p, m.n);
    } else if (cmd == "spawn" && argc > 2) {
        std::vector<char> out;
        if ((ok = capture_stdout(std::vector<std::string>(argv + 2, argv + argc), &out, &err))) print_bytes(out.data(), out.size());
    } else {
        fprintf(stderr, "usage: run_files_check region|bed|indel_regions|map|spawn ...\n");
        return 2;
    }
    if (!ok) printf("error: %s\n", err.c_str());
    return 0;
}
