// GPU-free half of the BAM front end the device consumers share (pipeline.hip, pileup.hip, allelecount.hip): the layout of a
// several-part upload block, the tables that turn one span's BGZF blocks and the .bai's virtual offsets into offsets of one linear
// record stream, and the index query with its growing table.  Standard library and the C header only, so that a plain C++ compiler -
// and a sanitizer - sees it (tests/host/bam_span_check.cpp).  The device half is inflated_span.h and RecordStream in bam_records.h.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../include/clairsto_amd.h"

namespace cto {

// Up to MAX parts that travel as ONE copy: every part starts 256-byte aligned and has at least 256 bytes behind it that belong to
// nobody (kernels that read a part in wide words may run over its end).
struct UploadParts {
    static constexpr int MAX = 8;
    int n = 0;
    const void* src[MAX];
    size_t bytes[MAX], off[MAX], total = 0;
    int add(const void* p, size_t b) {   // -> the part's index
        src[n] = p; bytes[n] = b; off[n] = total;
        total += (b + 255) / 256 * 256 + 256;
        return n++;
    }
    void stage(char* pinned, int first = 0) const {      // parts first.. into page-locked memory laid out like the device's
        for (int i = first; i < n; ++i) if (bytes[i]) memcpy(pinned + off[i], src[i], bytes[i]);
    }
    template <class T> T* at(void* base, int i) const { return reinterpret_cast<T*>(static_cast<char*>(base) + off[i]); }
};

// One span's blocks laid end to end: lin_off[b] = where block b's inflated bytes start in the linear stream (n_blocks + 1 entries),
// len = its length; starts = the virtual offsets that name a byte of the span, as linear offsets, ascending and distinct, with `len`
// as sentinel behind the n_chains of them.  An offset is kept when its block is in the table and it does not point past that block's
// inflated size (uoff == isize is the next block's first byte).  Nothing here is an error: limits are the callers'.
struct SpanTables {
    std::vector<int64_t> lin_off, starts;
    int64_t len = 0;
    int n_chains = 0;
    // in two steps, for the caller that has to look at `len` before it asks the index for the offsets
    void lay_out(const cto_bgzf_block* blocks, int64_t n_blocks) {
        lin_off.assign(size_t(n_blocks) + 1, 0);
        for (int64_t b = 0; b < n_blocks; ++b) lin_off[size_t(b) + 1] = lin_off[size_t(b)] + blocks[b].isize;
        len = lin_off[size_t(n_blocks)];
    }
    void map_starts(const cto_bgzf_block* blocks, int64_t n_blocks, const uint64_t* voffs, int64_t n_voffs) {
        starts.clear();
        for (int64_t i = 0; i < n_voffs; ++i) {
            const int64_t coff = int64_t(voffs[i] >> 16), uoff = int64_t(voffs[i] & 0xffff);
            int64_t lo = 0, hi = n_blocks;
            while (lo < hi) { const int64_t m = (lo + hi) / 2; if (int64_t(blocks[m].file_off) < coff) lo = m + 1; else hi = m; }
            if (lo >= n_blocks || int64_t(blocks[lo].file_off) != coff || uoff > int64_t(blocks[lo].isize)) continue;     // outside the span
            starts.push_back(lin_off[size_t(lo)] + uoff);
        }
        std::sort(starts.begin(), starts.end());
        starts.erase(std::unique(starts.begin(), starts.end()), starts.end());
        n_chains = int(starts.size());
        starts.push_back(len);
    }
};

// cto_bam_record_starts with a table that grows (x 8, four tries) while the index names more offsets than it holds.  Returns what
// the last call returned: the number of offsets now in `voffs`, or its error - CTO_ENOMEM when even the last table was too small.
inline int64_t record_starts(const char* bam_path, const char* bai_path, const char* ctg_name, int64_t start, int64_t end, int64_t file_begin,
                             int64_t file_end, std::vector<uint64_t>* voffs, int32_t* tid) {
    voffs->resize(size_t(4096 + ((end - start) >> 14) + 64));
    int64_t n = CTO_ENOMEM;
    for (int tries = 0; tries < 4 && n == CTO_ENOMEM; ++tries) {
        if (tries) voffs->resize(voffs->size() * 8);
        n = cto_bam_record_starts(bam_path, bai_path, ctg_name, start, end, file_begin, file_end, voffs->data(), int64_t(voffs->size()), tid);
    }
    return n;
}

}  // namespace cto
