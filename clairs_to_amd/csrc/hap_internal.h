// What the producers of a haplotype-filter job (csrc/hapfilter.cpp) share: the raw columns a BAM producer hands to the job builder
// (the host rules: csrc/bam.cpp; the device path and the C entry point: csrc/hapwindows.hip) and the builder itself.  Standard library
// only: the host rules are seen by a plain C++ compiler.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace cto {

// One printed base of a column.  `read` indexes HapRaw::names / hp: the entered read whose NAME, HP, BQ and MQ the record carries -
// behind a reference skip that is the cover one place ahead of the read the base came from, as the text pairs them.
struct HapRawRec {
    int32_t read;
    uint8_t base;                // as printed: A C G T N a c g t n * #
    uint8_t bq, mq;              // capped at 93
    uint8_t mark;                // 1: the read's first reference position (^), 2: its last ($); only read by hap_rse_from_marks
    int32_t indel_off, indel_len;      // into HapRaw::indel: sign + sequence in printed case, no digits; 0 / 0 when none
};

// Columns in ascending position, records of a column in file order of the entered reads (CSR).
struct HapRaw {
    std::vector<int64_t> col_pos;      // 1-based
    std::vector<int64_t> col_off;      // n_cols + 1
    std::vector<HapRawRec> recs;
    std::vector<int64_t> rse_off;      // n_cols + 1: the column's start / end index list (parse_row's indices, -1 = "the last record")
    std::vector<int32_t> rse;
    std::string indel;
    std::vector<std::string> names;    // per entered read: QNAME
    std::vector<uint8_t> hp;           // per entered read: k_hp_class's 0 (untagged), 1, 2, 3 (the value 12: prints two characters)
    void clear() { col_pos.clear(); col_off.assign(1, 0); recs.clear(); rse_off.assign(1, 0); rse.clear(); indel.clear(); names.clear(); hp.clear(); }
};

// parse_row's start / end sets of a column whose covers all print (no reference skip): a head record at index i gives i - 1 to the
// start set, a tail record i to the end set; the larger set wins, the end set on a tie.  Appends to `out` (ascending).
inline void hap_rse_from_marks(const HapRawRec* r, int64_t n, std::vector<int32_t>* out) {
    int64_t ns = 0, ne = 0;
    for (int64_t i = 0; i < n; ++i) { ns += r[i].mark & 1; ne += (r[i].mark >> 1) & 1; }
    const bool starts = ns > ne;
    for (int64_t i = 0; i < n; ++i)
        if (r[i].mark & (starts ? 1 : 2)) out->push_back(int32_t(starts ? i - 1 : i));
}

struct HapWinParams { int min_mq, min_bq, excl_flags, max_depth, reverse_del; };

// The host rules (csrc/bam.cpp): the columns of the 0-based, ascending, disjoint intervals iv[0 .. n_iv) [s, e) inside -r ctg:lo-hi,
// appended to *raw (which the caller cleared).  *n_entered: the reads that entered the pile-up of the region.
int hap_windows_host(const char* bam_path, const char* bai_path, const char* ctg_name, int64_t region_lo, int64_t region_hi, const int64_t* iv,
                     int64_t n_iv, const HapWinParams& pr, HapRaw* raw, int64_t* n_entered);

// The job builder (csrc/hapfilter.cpp): an empty job over [lo, hi] (cto_hap_job_free releases it); hap_job_add appends columns
// [c0, c1) of `raw` - all behind the columns already there - interning the "<qname>_<0|1>" keys, the suffix from the printed
// character, and the Counter keys.
int hap_job_new(int64_t lo, int64_t hi, void** job);
int hap_job_add(void* job, const HapRaw& raw, int64_t c0, int64_t c1);

}  // namespace cto
