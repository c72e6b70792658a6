// GPU-free file handling of the native chunk pipeline (pipeline.hip): files mapped or inflated into memory, a child's stdout, the
// FASTA index and a region of the reference, BED rows as merged intervals, the thread queue and the two clocks.  Standard library,
// POSIX and zlib only, so that a plain C++ compiler - and a sanitizer - sees it (tests/host/run_files_check.cpp).
#pragma once
#include <fcntl.h>
#include <spawn.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <time.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

extern char** environ;

namespace cto {
namespace run_files {

inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
inline double cpu_s() { timespec ts; clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts); return double(ts.tv_sec) + double(ts.tv_nsec) * 1e-9; }   // this thread's CPU time

template <class T>
struct Queue {                            // unbounded MPMC queue with a closed state
    std::mutex m;
    std::condition_variable cv;
    std::deque<T> q;
    bool closed = false;
    void push(T v) { { std::lock_guard<std::mutex> g(m); q.push_back(std::move(v)); } cv.notify_one(); }
    void close() { { std::lock_guard<std::mutex> g(m); closed = true; } cv.notify_all(); }
    // the next entry: waits for one until the queue is closed (ms < 0), for `ms` milliseconds, or not at all (0)
    bool pop(T* out, int ms = -1) {
        std::unique_lock<std::mutex> g(m);
        const auto ready = [&] { return !q.empty() || closed; };
        if (ms < 0) cv.wait(g, ready);
        else if (ms > 0) cv.wait_for(g, std::chrono::milliseconds(ms), ready);
        if (q.empty()) return false;
        *out = std::move(q.front());
        q.pop_front();
        return true;
    }
};

struct File {                             // a read-only descriptor that goes with its scope
    int fd;
    explicit File(const char* path) : fd(::open(path, O_RDONLY | O_CLOEXEC)) {}
    File(const File&) = delete; File& operator=(const File&) = delete;
    ~File() { if (fd >= 0) ::close(fd); }
    bool ok() const { return fd >= 0; }
    bool size(size_t* n) const { struct stat st; if (fstat(fd, &st) != 0) return false; *n = size_t(st.st_size); return true; }
};

// `n` bytes of `fd` from `offset` on into `buf`; false: the file ends (or a read fails) before that
inline bool read_exact(int fd, void* buf, size_t n, int64_t offset) {
    size_t got = 0;
    while (got < n) {
        const ssize_t r = pread(fd, static_cast<char*>(buf) + got, n - got, off_t(offset) + off_t(got));
        if (r <= 0) break;
        got += size_t(r);
    }
    return got == n;
}

struct Mapped {                           // a file's bytes: mapped read-only, or - for a *.gz path - inflated into memory (zlib)
    const char* p = nullptr;
    size_t n = 0;
    std::vector<char> owned;
    Mapped() = default;
    Mapped(const Mapped&) = delete; Mapped& operator=(const Mapped&) = delete;
    // sniff = true: look at the first two bytes instead of the name (`gzip -fdc`, which the reference's bed_tree_from pipes every BED
    // through, shared/interval_tree.py:43, inflates what is gzip and passes on what is not)
    bool open(const char* path, std::string* err, bool sniff = false) {
        const size_t pl = strlen(path);
        bool gz = pl > 3 && strcmp(path + pl - 3, ".gz") == 0;        // the reference's readers gzip.open such files
        if (sniff && !gz) {
            const File f(path);
            if (!f.ok()) { *err = std::string("cannot open ") + path; return false; }
            unsigned char magic[2] = {0, 0};
            gz = ::read(f.fd, magic, 2) == 2 && magic[0] == 0x1f && magic[1] == 0x8b;
        }
        if (gz) {
            gzFile g = gzopen(path, "rb");
            if (!g) { *err = std::string("cannot open ") + path; return false; }
            (void)gzbuffer(g, 1 << 20);
            owned.resize(size_t(1) << 22);
            size_t got = 0;
            for (;;) {
                if (got == owned.size()) owned.resize(owned.size() * 2);
                const int r = gzread(g, owned.data() + got, unsigned(std::min<size_t>(owned.size() - got, size_t(1) << 30)));
                if (r < 0) { gzclose(g); *err = std::string("cannot inflate ") + path; return false; }
                if (r == 0) break;
                got += size_t(r);
            }
            gzclose(g);
            owned.resize(got);
            p = got ? owned.data() : nullptr;
            n = got;
            return true;
        }
        const File f(path);
        if (!f.ok()) { *err = std::string("cannot open ") + path; return false; }
        if (!f.size(&n)) { n = 0; *err = std::string("cannot stat ") + path; return false; }
        if (n) {
            void* m = mmap(nullptr, n, PROT_READ, MAP_PRIVATE, f.fd, 0);
            if (m == MAP_FAILED) { n = 0; *err = std::string("cannot map ") + path; return false; }
            p = static_cast<const char*>(m);
        }
        return true;
    }
    ~Mapped() { if (p && n && owned.empty()) munmap(const_cast<char*>(p), n); }
};

// stdout of `argv` (a `samtools mpileup ...` command line) into `out`; false + *err when it cannot be started or exits non-zero
// (create_tensor_pileup_calling.py:426-446 pipes the same command; subprocess.run(check=True) in the Python mirror)
inline bool capture_stdout(const std::vector<std::string>& argv, std::vector<char>* out, std::string* err) {
    int fds[2];
    if (pipe2(fds, O_CLOEXEC) != 0) { *err = "pipe() failed"; return false; }
    posix_spawn_file_actions_t fa;
    posix_spawn_file_actions_init(&fa);
    posix_spawn_file_actions_adddup2(&fa, fds[1], 1);
    std::vector<char*> av;
    for (const std::string& a : argv) av.push_back(const_cast<char*>(a.c_str()));
    av.push_back(nullptr);
    pid_t pid = 0;
    const int rc = posix_spawnp(&pid, av[0], &fa, nullptr, av.data(), environ);
    posix_spawn_file_actions_destroy(&fa);
    ::close(fds[1]);
    if (rc != 0) { ::close(fds[0]); *err = "cannot run " + argv[0] + ": " + strerror(rc); return false; }
    out->clear();
    out->resize(size_t(1) << 22);
    size_t got = 0;
    for (;;) {
        if (got == out->size()) out->resize(out->size() * 2);
        const ssize_t r = read(fds[0], out->data() + got, out->size() - got);
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) break;
        got += size_t(r);
    }
    ::close(fds[0]);
    out->resize(got);
    int status = 0;
    while (waitpid(pid, &status, 0) < 0 && errno == EINTR) {}
    if (!WIFEXITED(status) || WEXITSTATUS(status) != 0) {
        *err = argv[0] + " mpileup failed (exit status " + std::to_string(WIFEXITED(status) ? WEXITSTATUS(status) : -1) + ")";
        return false;
    }
    return true;
}

struct FaiRec { int64_t length = 0, offset = 0, linebases = 0, linewidth = 0; bool ok = false; };

// <fasta>.fai (or <fasta without extension>.fai): the record of contig `ctg`  (fasta.py read_region)
inline bool fai_lookup(const std::string& fasta, const std::string& ctg, FaiRec* rec, std::string* err) {
    std::string fai = fasta + ".fai";
    FILE* f = fopen(fai.c_str(), "r");
    if (!f) {
        const size_t dot = fasta.rfind('.');
        if (dot != std::string::npos) { fai = fasta.substr(0, dot) + ".fai"; f = fopen(fai.c_str(), "r"); }
    }
    if (!f) { *err = "[ERROR] file " + fasta + ".fai not found"; return false; }
    char line[4096];
    while (fgets(line, sizeof(line), f)) {
        char* tab = strchr(line, '\t');
        if (!tab) continue;
        if (size_t(tab - line) == ctg.size() && memcmp(line, ctg.data(), ctg.size()) == 0) {
            long long a = 0, b = 0, c = 0, d = 0;
            if (sscanf(tab + 1, "%lld\t%lld\t%lld\t%lld", &a, &b, &c, &d) == 4 && c > 0 && d > 0) {
                rec->length = a; rec->offset = b; rec->linebases = c; rec->linewidth = d; rec->ok = true;
            }
            break;
        }
    }
    fclose(f);
    if (!rec->ok) { *err = "contig " + ctg + " not in " + fai; return false; }
    return true;
}

// 1-based inclusive [start, end] of the contig, upper-cased, clipped to the contig (fasta.py read_region)
inline bool read_region(const Mapped& fa, const FaiRec& r, int64_t start, int64_t end, std::string* out, std::string* err) {
    out->clear();
    if (fa.n >= 2 && (unsigned char)fa.p[0] == 0x1f && (unsigned char)fa.p[1] == 0x8b) {
        *err = "[ERROR] the reference is gzip / bgzip compressed: decompress it (and re-run samtools faidx) before use";
        return false;
    }
    start = std::max<int64_t>(1, start);
    end = std::min<int64_t>(r.length, end);
    if (end < start) return true;
    const int64_t s0 = start - 1, e0 = end;
    const int64_t b0 = r.offset + (s0 / r.linebases) * r.linewidth + s0 % r.linebases;
    const int64_t b1 = r.offset + ((e0 - 1) / r.linebases) * r.linewidth + (e0 - 1) % r.linebases + 1;
    if (b0 < 0 || b1 > int64_t(fa.n) || b1 < b0) { *err = "reference index points outside the FASTA file"; return false; }
    out->resize(size_t(end - start + 1));
    char* dst = &(*out)[0];
    size_t n = 0;
    for (const char* q = fa.p + b0; q < fa.p + b1;) {                 // line by line: memchr + one pass that folds the case
        const char* nl = static_cast<const char*>(memchr(q, '\n', size_t(fa.p + b1 - q)));
        const char* e = nl ? nl : fa.p + b1;
        for (const char* c = q; c < e; ++c)
            if (*c != '\r' && n < out->size()) dst[n++] = (*c >= 'a' && *c <= 'z') ? char(*c - 32) : *c;
        q = e + 1;
    }
    out->resize(n);
    return true;
}

// [begin, end) pairs -> sorted, overlapping and touching ones merged, flat: begin0, end0, begin1, end1, ...
inline void merge_intervals(std::vector<std::pair<int64_t, int64_t>>* iv, std::vector<int64_t>* out) {
    std::sort(iv->begin(), iv->end());
    out->clear();
    for (const auto& p : *iv) {
        if (!out->empty() && p.first <= out->back()) out->back() = std::max(out->back(), p.second);
        else { out->push_back(p.first); out->push_back(p.second); }
    }
}

// BED rows of `ctg` as 0-based [begin, end) intervals, sorted and merged (what `samtools mpileup -l` restricts positions to)
inline void bed_intervals(const char* text, size_t len, const std::string& ctg, std::vector<int64_t>* out) {
    std::vector<std::pair<int64_t, int64_t>> iv;
    size_t i = 0;
    while (i < len) {
        const char* nl = static_cast<const char*>(memchr(text + i, '\n', len - i));
        const size_t e = nl ? size_t(nl - text) : len;
        const char* row = text + i;
        const size_t rl = e - i;
        const char* t1 = static_cast<const char*>(memchr(row, '\t', rl));
        if (t1 && size_t(t1 - row) == ctg.size() && memcmp(row, ctg.data(), ctg.size()) == 0) {
            const char* t2 = static_cast<const char*>(memchr(t1 + 1, '\t', rl - size_t(t1 + 1 - row)));
            if (t2) {
                const long long a = atoll(std::string(t1 + 1, size_t(t2 - t1 - 1)).c_str());
                const char* t3 = static_cast<const char*>(memchr(t2 + 1, '\t', rl - size_t(t2 + 1 - row)));
                const size_t l3 = t3 ? size_t(t3 - t2 - 1) : rl - size_t(t2 + 1 - row);
                const long long b = atoll(std::string(t2 + 1, l3).c_str());
                iv.emplace_back(std::max<long long>(0, a), b);
            }
        }
        i = e + 1;
    }
    merge_intervals(&iv, out);
}

// --call_indels_only_in_these_regions: per contig the rows of the BED at `path` (plain or gzip, whatever its name) as sorted, merged
// [begin, end) intervals (bed_tree_from of the reference)
inline bool load_indel_regions(const char* path, std::map<std::string, std::vector<int64_t>>* out, std::string* err) {
    Mapped bed;
    if (!bed.open(path, err, /*sniff=*/true)) return false;
    std::map<std::string, std::vector<std::pair<int64_t, int64_t>>> rows;
    size_t i = 0;
    int64_t row_id = 0;
    while (i < bed.n) {
        ++row_id;
        const char* nl = static_cast<const char*>(memchr(bed.p + i, '\n', bed.n - i));
        const size_t e = nl ? size_t(nl - bed.p) : bed.n;
        std::string row(bed.p + i, e - i);
        i = e + 1;
        if (row.empty() || row[0] == '#') continue;
        char name[256];
        long long a = 0, b = 0;
        if (row.find_first_not_of(" \t\r") == std::string::npos) continue;
        // a row the reference cannot split into name, start, end ends its run with an exception (interval_tree.py:47-55): an
        // unreadable BED must not turn into "no regions", which would let every indel candidate through
        if (sscanf(row.c_str(), "%255s %lld %lld", name, &a, &b) != 3) {
            *err = "[ERROR] Invalid bed input in " + std::to_string(row_id) + "-th row of " + std::string(path) + ": " + row.substr(0, 80);
            return false;
        }
        if (b < a || a < 0 || b < 0) { *err = "[ERROR] Invalid bed input in " + std::string(path) + ": " + row; return false; }
        if (a == b) ++b;
        rows[name].emplace_back(a, b);
    }
    for (auto& kv : rows) merge_intervals(&kv.second, &(*out)[kv.first]);
    return true;
}

}  // namespace run_files
}  // namespace cto
