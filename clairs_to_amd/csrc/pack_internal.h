// Internals shared by the two pack producers (mpileup text: pack.cpp, BAM: bam.cpp): the pack object and the per-column
// appender that turns a column's read-bases into entries + distinct indel keys.
#pragma once
#include <algorithm>
#include <memory>
#include <new>
#include <exception>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>
#include "common.h"

// resize() without the zero fill: the entry array (tens of MB per chunk) is always overwritten right after it is grown - by
// the tokeniser's single pass and by the threads of the parallel merge
template <class T>
struct default_init_alloc : std::allocator<T> {
    template <class U> struct rebind { using other = default_init_alloc<U>; };
    template <class U, class... A>
    void construct(U* p, A&&... a) {
        if constexpr (sizeof...(A) == 0) ::new (static_cast<void*>(p)) U;
        else ::new (static_cast<void*>(p)) U(std::forward<A>(a)...);
    }
};

struct cto_pack {
    std::vector<int32_t> col_pos;
    std::vector<uint8_t> col_ref;
    std::vector<int64_t> col_off;   // n_cols + 1
    std::vector<int32_t> key_off;   // n_cols + 1
    std::vector<uint32_t, default_init_alloc<uint32_t>> entries;
    // Entry array in memory the caller owns (the chunk pipeline's page-locked staging buffer): the merge of the tokeniser's
    // per-thread parts writes there directly and `entries` stays empty.  The caller keeps it alive as long as the pack.
    uint32_t* ext_entries = nullptr;
    size_t ext_n = 0;
    std::vector<uint8_t> key_meta;
    std::vector<int32_t> key_group;
    std::vector<int64_t> key_str_off;  // n_keys + 1
    std::string key_str;               // alt_info keys ("I<ANCHOR><SEQ>", "D<refslice>")
};


namespace cto {

inline char up(char c) { return (c >= 'a' && c <= 'z') ? char(c - 32) : c; }

inline int base_code(char c) {
    switch (c) {
        case 'A': return 0;  case 'C': return 1;  case 'G': return 2;  case 'T': return 3;
        case 'a': return 4;  case 'c': return 5;  case 'g': return 6;  case 't': return 7;
        case '*': return 8;  case '#': return 9;  case 'N': return 10; case 'n': return 11;
        default:  return -1;
    }
}

// evc_base_from(...).upper(): ACGT (any case) stay, everything else becomes 'A'.
inline int ref_code_of(char c) {
    switch (up(c)) {
        case 'A': return 0; case 'C': return 1; case 'G': return 2; case 'T': return 3;
        default:  return 0;
    }
}

struct Tok {
    int code;          // base code
    int kind;          // 0 none, 1 ins, 2 del
    const char* seq;   // indel sequence as mpileup prints it (not owned): inserted bases in the strand's case, N/n for deletions
    int seqlen;
    int bq, mq;        // phred values
};

constexpr int kMaxDepth = 32767;
constexpr int kMaxKeysPerCol = 2048;

// Distinct indel keys of the column being built.  A column has a handful of them, so the look-up is a scan over 32-bit hashes
// (a hit is confirmed on the characters); the sequences stay where the producer has them (mpileup text / BAM record) for the
// duration of the column.  (std::string keys in two hash maps cost ~150 ns per indel-carrying read-base - a third of the
// tokeniser's time on 50x long-read rows.)
struct ColumnScratch {
    struct Key   { const char* seq; int len; uint8_t code, kind; };     // Counter key: base character + sign + sequence, case-sensitive
    struct Group { const char* seq; int len; char anchor; uint8_t kind; };   // merged allele: anchor + upper-cased sequence / deletion length
    std::vector<uint32_t> key_hash, group_hash;
    std::vector<Key> keys;
    std::vector<Group> groups;
};

// Decoding threads of the pack producers for calls made from THIS thread (0: CTO_PACK_THREADS, else the producer's default): the chunk
// pipeline sets it in its producer threads, so that nobody has to edit the process environment around a call.
extern thread_local int tl_pack_threads;
inline unsigned pack_threads_or(unsigned dflt) {
    if (tl_pack_threads > 0) return unsigned(std::min(tl_pack_threads, 64));
    if (const char* e = getenv("CTO_PACK_THREADS")) return std::max(1u, std::min(unsigned(atoi(e)), 64u));
    return dflt;
}

// No C++ exception crosses the C ABI (or leaves a worker thread): allocation failures on hostile input come back as error codes.
template <class F>
int guarded(const char* what, F&& f) {
    try {
        return f();
    } catch (const std::bad_alloc&) {
        set_error("%s: out of memory", what);
        return CTO_ENOMEM;
    } catch (const std::exception& e) {
        set_error("%s: %s", what, e.what());
        return CTO_EINVAL;
    } catch (...) {
        set_error("%s: unknown failure", what);
        return CTO_EINVAL;
    }
}

void set_err(std::string* err, const char* fmt, ...);
void pack_begin(cto_pack* p, size_t entries_hint, size_t cols_hint);
// Appends one column (position `pos`, reference index ri = pos - ref_start) made of toks[0..n)
int append_column(cto_pack* p, ColumnScratch& sc, int64_t pos, int64_t ri, const char* ref_seq, size_t ref_len,
                  int max_indel_length, const Tok* toks, int n, std::string* err);

// The same for a producer that packs the plain read-bases itself: ents[0..n) are finished entries (code | bq << 6 | mq << 13)
// except at the indices named by indels[0..n_indel), whose kind / key id are filled in here.
struct IndelAt {
    int idx;           // index into ents
    int kind;          // 1 ins, 2 del
    const char* seq;
    int seqlen;
};
inline uint32_t pack_entry(int code, int bq, int mq) { return uint32_t(code) | (uint32_t(bq) << 6) | (uint32_t(mq) << 13); }
int append_column_packed(cto_pack* p, ColumnScratch& sc, int64_t pos, int64_t ri, const char* ref_seq, size_t ref_len,
                         int max_indel_length, const uint32_t* ents, int n, const IndelAt* indels, int n_indel, std::string* err);

std::unique_ptr<cto_pack> merge_parts(std::vector<std::unique_ptr<cto_pack>>& parts, std::string* err, uint32_t* ext_entries = nullptr,
                                      size_t ext_cap = 0);
// cto_pack_from_mpileup with the entry array placed in ext_entries[0 .. ext_cap) when it fits (see cto_pack::ext_entries)
int pack_from_mpileup_impl(const char* text, size_t len, const char* ref_seq, int64_t ref_start, size_t ref_len, int max_indel_length,
                           uint32_t* ext_entries, size_t ext_cap, cto_pack** out);

// cto_extract_candidates with the caller's own overflow counters (scratch dev [n_keys] uint32): what concurrent callers on different
// streams use (csrc/pipeline.hip: one buffer per chunk slot); csrc/extract.hip
int extract_candidates_scratch(const cto_pack_view* dp, int min_mq, int min_bq, double snv_min_af, double indel_min_af, double min_coverage,
                               int alt_base_num, int select_indel, uint32_t* scratch, uint8_t* flags, int32_t* depth, void* stream);
// Allele counter (the C entry point and the device path: csrc/allelecount.hip; the host rules and the index-based chunk plan sit beside
// the pile-up producer, csrc/bam.cpp).  loci: 1-based, strictly ascending; counts: n_loci x 4 (A C G T), zeroed by the call.
struct AlleleParams { int min_bq, min_mq, req_flags, excl_flags; };
int allele_counts_host_range(const char* bam_path, const char* bai_path, const char* ctg_name, const int32_t* loci, int64_t n_loci,
                             const AlleleParams& pr, int32_t* counts, int64_t* n_entered, double* ms_records, double* ms_count);
int allele_plan_chunks(const char* bam_path, const char* bai_path, const char* ctg_name, const int32_t* loci, int64_t n_loci, int64_t budget,
                       std::vector<int64_t>* cuts);
// AF tallies (the C entry point, the rules and the device path: csrc/aftally.hip; the host rules: csrc/bam.cpp).  The arrays are the
// call's own, over all its loci; sel[0 .. n_sel) are the ascending indices of the loci to tally, and row sel[i] of `out` (n_loci x 8,
// zeroed for them by the call) receives the result.
struct AfLoci { const int32_t* pos; const uint8_t *kind, *base; const int32_t* del_len; const char* ins_bytes; const int64_t* ins_off; };
struct AfParams { int min_mq, excl_flags, max_depth, with_hp; };
int af_tallies_host_range(const char* bam_path, const char* bai_path, const char* ctg_name, const AfLoci& loci, const int64_t* sel, int64_t n_sel,
                          const AfParams& pr, int32_t* out, int64_t* n_entered, double* ms_records, double* ms_count);
// Read phasing (the C entry point, the rules and the device path: csrc/phase.hip; the host rules and the phase pass: csrc/bam.cpp).
// pos: 1-based, strictly ascending; ref / alt: one ASCII letter per site.  A read list is a CSR: reads in file order, named by the
// virtual offset of their record, each with its observations site * 2 + allele in ascending site order.
struct PhaseSites { const int32_t* pos; const uint8_t *ref, *alt; int64_t n; };
struct PhaseParams { int min_mq, excl_flags, link_span; };
struct PhaseReads { std::vector<uint64_t> voff; std::vector<int64_t> off{0}; std::vector<int32_t> obs; };
inline int phase_base_code(uint8_t letter) {             // the 4-bit code of a BAM sequence for A C G T (either case), 0 for anything else
    switch (letter & 0xdf) { case 'A': return 1; case 'C': return 2; case 'G': return 4; case 'T': return 8; default: return 0; }
}
int phase_observe_host_range(const char* bam_path, const char* bai_path, const char* ctg_name, const PhaseSites& S, int64_t a, int64_t b,
                             const PhaseParams& pr, PhaseReads* out, double* ms);
void phase_merge(const std::vector<PhaseReads>& parts, PhaseReads* out, int64_t* n_merged);
void phase_link_host(const PhaseReads& R, int64_t n, int K, int32_t* link);          // link: n x K x 2, zeroed by the call
void phase_sites(const int32_t* link, const int32_t* pos, int64_t n, int K, int8_t* phase, int32_t* ps, int32_t* block, int64_t* n_blocks);
void phase_assign_host(const PhaseReads& R, const int8_t* phase, const int32_t* block, const int32_t* ps, uint8_t* hp, int32_t* rps);
// Coverage, subsample and merge (the C entry points, the rules and the device path: csrc/contam.hip; the host rules, the window plan
// and the writer of the output BAM and its index: csrc/bam.cpp).  A window [w0, w1) is a run of 16 kb index windows of one contig and
// owns the records with w0 <= pos < w1.
constexpr int64_t kContamWindow = 16384;
constexpr int64_t kContamMaxWindows = 1024;              // per chunk: the depth array of a chunk stays within 16 Mi positions
constexpr int kCovExclFlags = 1796;                      // mosdepth's default: unmapped, secondary, QC fail, duplicate
struct BamHeader { std::vector<uint8_t> raw; std::vector<std::string> names; std::vector<int64_t> lens; };   // raw: magic .. reference list
int contam_read_header(const char* who, const char* bam_path, BamHeader* out);
// cuts: chunk boundaries in 16 kb windows, 0 .. ceil(L / 16384), so that four times the compressed bytes the sources' linear indices
// name between two cuts, plus one byte per window (a budget of 1 gives single windows), stay within `budget`
int contam_plan_windows(const char* who, const char* const* bams, const char* const* bais, int n_src, const char* ctg_name, int64_t L,
                        int64_t budget, std::vector<int64_t>* cuts);
// rule b: the 24 bits samtools compares with the fraction, from the read name's n bytes
inline uint32_t subsample_key(const uint8_t* name, int n, uint32_t seed) {
    uint32_t h = n > 0 ? name[0] : 0;
    for (int i = 1; i < n; ++i) h = h * 31u + name[i];
    uint32_t k = h ^ seed;
    k += ~(k << 15); k ^= k >> 10; k += k << 3; k ^= k >> 6; k += ~(k << 11); k ^= k >> 16;
    return k & 0xffffffu;
}
inline bool subsample_keeps(uint32_t k24, int m) { return uint64_t(k24) * 1000u < (uint64_t(uint32_t(m)) << 24); }
// carry: the clipped ends of the spans open at w0 on entry, at w1 on return; *mn / *mx over the window's positions inside the contig
int cov_window_host(const char* bam_path, const char* bai_path, const char* ctg_name, int64_t w0, int64_t w1, int64_t L, std::vector<int32_t>* carry,
                    int64_t* bases, int32_t* mn, int32_t* mx, int64_t* n_counted);
struct MixRow { int32_t pos, rlen, bin, pad_; int64_t off; };      // of a written record: what the index asks; off: in the window's stream
struct MixCounts { int64_t cand[2], kept[2]; };                    // [0] tumour, [1] normal
int mix_window_host(const char* const* bams, const char* const* bais, const char* ctg_name, int64_t w0, int64_t w1, const int* m, uint32_t seed,
                    std::vector<uint8_t>* stream, std::vector<MixRow>* rows, MixCounts* counts);
// The output file: header + the windows' streams cut into BGZF blocks of 0xff00 bytes, deflated on `threads` threads and written in
// order; close() writes the end block and <path>.bai from the rows.  coder: 0 zlib level 6; 1 csrc/deflate.hip on the device (bytes
// appended on the host go up and the blocks come down; append_coded takes blocks coded where the stream was built); 2 its host
// restatement on the threads.  1 and 2 write the same bytes.
struct MixWriter {
    struct Rec { int32_t tid, pos, rlen, bin; int64_t u0, u1; };
    FILE* f = nullptr;
    std::string path;
    int n_ref = 0, threads = 1;
    std::vector<uint8_t> pending;        // the stream's bytes behind the last block written
    int64_t u_pending = 0, file_off = 0; // stream offset of pending[0]; bytes written
    int64_t end_off = 0;                 // file offset of the empty end block
    std::vector<int64_t> coff;           // file offset of every block written
    std::vector<Rec> recs;
    double ms = 0;
    int coder = 0;
    void* stream = nullptr;              // hipStream_t of coder 1
    cto_deflate_stats dst{};
    ~MixWriter() { if (f) fclose(f); }
    int open(const char* out_path, const BamHeader& h, int n_threads, int deflate_mode = 0, void* hip_stream = nullptr);
    int append(int tid, const uint8_t* stream, size_t n, const MixRow* rows, size_t n_rows);
    // a window of n stream bytes whose whole blocks, counted from pending[0], are coded already: n_blocks blocks back to back in
    // `blocks`, and the n_rest bytes behind them, which become the new pending
    int append_coded(int tid, size_t n, const MixRow* rows, size_t n_rows, const uint32_t* sizes, size_t n_blocks, const uint8_t* blocks,
                     const uint8_t* rest, size_t n_rest);
    void add_rows(int tid, size_t n, const MixRow* rows, size_t n_rows);
    int close(int64_t* out_bytes, int64_t* out_blocks);
    int flush(bool all);
};
}  // namespace cto
