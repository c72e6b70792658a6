// add_back_missing_variants_in_genotyping (cto_add_back, include/clairsto_amd.h): the reference's src/add_back_missing_variants_in_genotyping.py
// from the bytes of its three inputs to the bytes of its output, on the device or - the same rules, plain C++ - on the host.
//
// The rules (derived in DESIGN.md "add_back"):
//   1  A text is cut into lines at '\n' only.  A VCF line (calls, list) is read by its whitespace tokens (str.strip().split()): a first token
//      that starts with '#' makes a header line, otherwise the key is (token 1, int(token 2)).  A line without two tokens ends the call
//      (bad_source / bad_line): the reference crashes on it.
//   2  The header lines of the calls, in file order, open the output, byte for byte.
//   3  Records go into dicts: of the lines with one key the LAST counts, in the calls and in the list alike.
//   4  An info line is read by its tab columns (rstrip('\n').split('\t')): fewer than four columns and it is skipped, otherwise the key is
//      (column 1, int(column 2)) and it carries ref_base (column 3) and the depth-seqs field (column 4); the last line of a key counts.
//   5  Genotyping mode emits exactly the list's keys: the calls' row where the key was called, else the list's row.  Hybrid mode emits
//      the calls' keys and the list's uncalled keys.
//   6  Rows are ordered by (contig rank, POS): the reference's 48 major contigs in its order, then every other contig in order of first
//      appearance (calls, then list).
//   7  A calls' row is copied byte for byte (a missing final newline stays missing); so is a list's row without switch_genotype.
//   8  With switch_genotype a list's row is rewritten: rstrip(), split at tabs, padded to 10 columns with '.'; REF becomes its first byte
//      ('.' when empty), replaced by a non-empty ref_base that differs; ALT QUAL FILTER INFO become '.', FORMAT GT:DP:AU:CU:GU:TU, the sample
//      ./.:DP:AU:CU:GU:TU; columns past the tenth stay; '\n' closes the row.
//   9  DP AU CU GU TU come from the depth-seqs field "<depth>-<key> <n> <key> <n> ...": not exactly one '-', or an int() that raises,
//      gives five zeros; keys pair with the numbers that follow them, the last A, C, G, T counts; an unpaired key is dropped.
//  10  The three counts: distinct list keys, distinct call keys, list keys that were not called.
//  11  Undecided, never guessed: a POS or a number of the field that is not 1-18 plain ASCII digits but holds a digit (int() may accept
//      '+5', '1_0', ' 7'), and a POS of 2^42 or more.  They are counted (stats->undecided) and nothing is written.  A text with '\r' or a
//      byte >= 0x80 (universal newlines, Unicode whitespace and digits) sets stats->non_ascii the same way.
//
// One sort does rules 3, 5 and 6: the records of the three sources, laid out calls, list, info in line order, are sorted stably by
// (rank << 42 | POS).  Equal keys form a run in which the calls' lines come first, then the list's, then the info's, each in file order,
// so "the last line of a key" is the last of its source in the run.
//
// Device passes: k_byte_class; per source k_line_count / scan / k_line_emit (lines.h); k_parse, one lane per line; k_heads marks the lines
// whose contig token differs bytewise from the line before, the host interns those few strings into ranks and k_keys spreads them through
// a scan of the marks; the sort (sort.h); k_runs, one lane per run; k_plan, one lane per output row (its length, and for a rewritten
// row its pieces and the five numbers); a scan of the lengths; k_compose, one wave per row.
#include <algorithm>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>
#include "hip_buffers.h"
#include "lines.h"
#include "sort.h"

using namespace cto;

namespace {

#define AB_HD __host__ __device__ __forceinline__

constexpr int POS_BITS = 42;
constexpr int64_t POS_LIMIT = int64_t(1) << POS_BITS;
constexpr uint32_t MAX_RANK = (1u << (64 - POS_BITS)) - 1;
enum : uint8_t { K_SKIP = 0, K_HEADER = 1, K_RECORD = 2, K_BAD = 3, K_UNDECIDED = 4 };
enum { SRC_CALLS = 0, SRC_LIST = 1, SRC_INFO = 2 };

struct Sources {                   // the three texts in one buffer, each at a multiple of 16
    uint32_t base[3], len[3];
    int64_t line0[4];              // the lines of source s are [line0[s], line0[s + 1])
};

struct Plan {                      // one output row
    uint32_t line_s, pre_len;      // kept row: the raw line; rewritten: its bytes up to the end of column 3 (or of the stripped line)
    uint32_t ref_s, ref_len;       // REF's bytes in the text; ref_len 0: '.'
    uint32_t tail_s, tail_len;     // from the tab before column 11 to the end of the stripped line
    uint32_t out_len;
    uint8_t rewritten, npad, undecided, pad_;
    int64_t v[5];
};

AB_HD bool is_ws(uint8_t c) { return c == ' ' || (c >= 9 && c <= 13) || (c >= 0x1c && c <= 0x1f); }      // str.strip() / str.split(), ASCII

// 0: 1-18 plain digits, *v their value; 1: int() raises (empty, or no digit in it); 2: undecided
AB_HD int plain_int(const uint8_t* t, uint32_t s, uint32_t e, int64_t* v) {
    bool plain = e > s && e - s <= 18, digit = false;
    int64_t x = 0;
    for (uint32_t i = s; i < e; ++i) {
        const uint8_t c = t[i];
        if (c >= '0' && c <= '9') { digit = true; if (plain) x = x * 10 + (c - '0'); }
        else plain = false;
    }
    if (plain) { *v = x; return 0; }
    return digit ? 2 : 1;
}

struct Parsed { uint8_t kind; uint32_t tok_s, tok_len, c3s, c3l, c4s, c4l; int64_t pos; };

// rule 1: [s, e) without the '\n'
AB_HD Parsed parse_vcf_line(const uint8_t* t, uint32_t s, uint32_t e) {
    Parsed p = {K_BAD, 0, 0, 0, 0, 0, 0, 0};
    uint32_t i = s;
    while (i < e && is_ws(t[i])) ++i;
    if (i == e) return p;
    if (t[i] == '#') { p.kind = K_HEADER; return p; }
    p.tok_s = i;
    while (i < e && !is_ws(t[i])) ++i;
    p.tok_len = i - p.tok_s;
    while (i < e && is_ws(t[i])) ++i;
    if (i == e) return p;
    const uint32_t q = i;
    while (i < e && !is_ws(t[i])) ++i;
    p.kind = plain_int(t, q, i, &p.pos) == 0 && p.pos < POS_LIMIT ? K_RECORD : K_UNDECIDED;
    return p;
}

// rule 4
AB_HD Parsed parse_info_line(const uint8_t* t, uint32_t s, uint32_t e) {
    Parsed p = {K_SKIP, s, 0, 0, 0, 0, 0, 0};
    uint32_t tab[4], n = 0;
    for (uint32_t i = s; i < e && n < 4; ++i) if (t[i] == '\t') tab[n++] = i;
    if (n < 3) return p;
    p.tok_len = tab[0] - s;
    p.c3s = tab[1] + 1; p.c3l = tab[2] - p.c3s;
    p.c4s = tab[2] + 1; p.c4l = (n == 4 ? tab[3] : e) - p.c4s;
    p.kind = plain_int(t, tab[0] + 1, tab[1], &p.pos) == 0 && p.pos < POS_LIMIT ? K_RECORD : K_UNDECIDED;
    return p;
}

// rule 9 on the field [s, e): false when undecided
AB_HD bool alt_info(const uint8_t* t, uint32_t s, uint32_t e, int64_t (&v)[5]) {
    for (int k = 0; k < 5; ++k) v[k] = 0;
    if (s == e) return true;
    uint32_t dash = e, dashes = 0;
    for (uint32_t i = s; i < e; ++i) if (t[i] == '-') { if (!dashes) dash = i; ++dashes; }
    if (dashes != 1) return true;
    bool raises = false, undecided = false;
    int64_t got[5] = {0, 0, 0, 0, 0};
    uint32_t item = dash + 1, key_s = 0, key_len = 0;
    for (uint32_t i = dash + 1, idx = 0; i <= e; ++i) {
        if (i < e && t[i] != ' ') continue;
        if (idx & 1) {
            int64_t x = 0;
            const int c = plain_int(t, item, i, &x);
            if (c == 1) raises = true;
            else if (c == 2) undecided = true;
            else if (key_len == 1) {
                const uint8_t b = t[key_s];
                const int at = b == 'A' ? 1 : b == 'C' ? 2 : b == 'G' ? 3 : b == 'T' ? 4 : 0;
                if (at) got[at] = x;
            }
        } else {
            key_s = item; key_len = i - item;
        }
        item = i + 1;
        ++idx;
    }
    const int c = plain_int(t, s, dash, &got[0]);
    if (c == 1) raises = true;
    else if (c == 2) undecided = true;
    if (raises) return true;
    if (undecided) return false;
    for (int k = 0; k < 5; ++k) v[k] = got[k];
    return true;
}

AB_HD uint32_t digits_of(int64_t x) { uint32_t n = 1; while (x >= 10) { x /= 10; ++n; } return n; }

constexpr int MID_LEN = 30;        // "\t.\t.\t.\t.\tGT:DP:AU:CU:GU:TU\t./."
AB_HD uint8_t mid_byte(int i) { const char* m = "\t.\t.\t.\t.\tGT:DP:AU:CU:GU:TU\t./."; return uint8_t(m[i]); }

// rule 7: the raw line [s, raw_e)
AB_HD Plan plan_kept(uint32_t s, uint32_t raw_e) {
    Plan p = {};
    p.line_s = s;
    p.pre_len = p.out_len = raw_e - s;
    return p;
}

// rule 8: the list's line [s, e) (without its '\n') and the info line's two fields (has_info)
AB_HD Plan plan_rewrite(const uint8_t* t, uint32_t s, uint32_t e, bool has_info, uint32_t c3s, uint32_t c3l, uint32_t c4s, uint32_t c4l) {
    Plan p = {};
    p.rewritten = 1;
    p.line_s = s;
    while (e > s && is_ws(t[e - 1])) --e;                  // rstrip()
    uint32_t ntab = 0, tab3 = e, tab4 = e, tab10 = e;      // the tabs that close columns 3, 4 and 10
    for (uint32_t i = s; i < e; ++i)
        if (t[i] == '\t') {
            ++ntab;
            if (ntab == 3) tab3 = i;
            else if (ntab == 4) tab4 = i;
            else if (ntab == 10) { tab10 = i; break; }
        }
    const uint32_t ncol = ntab + 1;                        // (at least 10 when the loop broke off)
    p.pre_len = tab3 - s;
    p.npad = uint8_t(ncol < 3 ? 3 - ncol : 0);
    if (ncol >= 4 && tab4 > tab3 + 1) { p.ref_s = tab3 + 1; p.ref_len = 1; }
    if (has_info && c3l > 0 && !(c3l == 1 && p.ref_len == 1 && t[c3s] == t[p.ref_s]) && !(c3l == 1 && p.ref_len == 0 && t[c3s] == '.')) {
        p.ref_s = c3s; p.ref_len = c3l;
    }
    if (ntab >= 10) { p.tail_s = tab10; p.tail_len = e - tab10; }
    if (has_info) p.undecided = alt_info(t, c4s, c4s + c4l, p.v) ? 0 : 1;
    p.out_len = p.pre_len + 2u * p.npad + 1 + (p.ref_len ? p.ref_len : 1) + MID_LEN + p.tail_len + 1;
    for (int k = 0; k < 5; ++k) p.out_len += 1 + digits_of(p.v[k]);
    return p;
}

// the bytes of a rewritten row between its prefix and its tail, but for REF's own: one thread
AB_HD void write_small(const Plan& p, uint8_t* o) {
    uint32_t at = p.pre_len;
    for (int k = 0; k < p.npad; ++k) { o[at++] = '\t'; o[at++] = '.'; }
    o[at++] = '\t';
    if (!p.ref_len) o[at] = '.';
    at += p.ref_len ? p.ref_len : 1;
    for (int i = 0; i < MID_LEN; ++i) o[at++] = mid_byte(i);
    for (int k = 0; k < 5; ++k) {
        o[at++] = ':';
        const uint32_t n = digits_of(p.v[k]);
        int64_t x = p.v[k];
        for (uint32_t j = n; j-- > 0;) { o[at + j] = uint8_t('0' + x % 10); x /= 10; }
        at += n;
    }
    o[at + p.tail_len] = '\n';
}
AB_HD uint32_t ref_at(const Plan& p) { return p.pre_len + 2u * p.npad + 1; }
AB_HD uint32_t tail_at(const Plan& p) { return p.out_len - 1 - p.tail_len; }

AB_HD int source_of(const Sources& S, int64_t line) { return line < S.line0[1] ? SRC_CALLS : line < S.line0[2] ? SRC_LIST : SRC_INFO; }

// what a run of equal keys decides (rules 3, 5): lines are sorted positions' payloads
struct RunPick { int64_t call, list, info; };

// ------------------------------------------------------------------------------------------------ kernels
struct DevStatus { unsigned long long non_ascii, undecided, first_bad, max_pos, counts[3]; };

__global__ __launch_bounds__(256) void k_byte_class(const uint8_t* __restrict__ text, uint32_t n, DevStatus* st) {
    const uint32_t i0 = (blockIdx.x * 256u + threadIdx.x) * 16u;
    if (i0 >= n) return;
    bool hit = false;
    if (i0 + 16 <= n) {
        const uint4 v = *reinterpret_cast<const uint4*>(text + i0);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 16; ++k) { const uint8_t b = uint8_t(w[k >> 2] >> (8 * (k & 3))); hit |= b == '\r' || b >= 0x80; }
    } else {
        for (uint32_t i = i0; i < n; ++i) hit |= text[i] == '\r' || text[i] >= 0x80;
    }
    if (hit) atomicOr(&st->non_ascii, 1ull);
}

struct LineArrays {
    uint32_t* start;               // per line, relative to its source (k_line_emit)
    uint8_t* kind;
    uint32_t *tok_s, *tok_len;
    int64_t* pos;
    uint32_t* info_cols;           // per info line: c3s, c3l, c4s, c4l
    int *is_rec, *is_head;
};

__device__ __forceinline__ void line_span(const Sources& S, const uint32_t* start, int64_t i, int src, uint32_t* s, uint32_t* raw_e) {
    *s = S.base[src] + start[i];
    *raw_e = S.base[src] + (i + 1 < S.line0[src + 1] ? start[i + 1] : S.len[src]);
}

__global__ __launch_bounds__(256) void k_parse(const uint8_t* __restrict__ text, Sources S, LineArrays A, DevStatus* st) {
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= S.line0[3]) return;
    const int src = source_of(S, i);
    uint32_t s, raw_e;
    line_span(S, A.start, i, src, &s, &raw_e);
    const uint32_t e = raw_e > s && text[raw_e - 1] == '\n' ? raw_e - 1 : raw_e;
    const Parsed p = src == SRC_INFO ? parse_info_line(text, s, e) : parse_vcf_line(text, s, e);
    A.kind[i] = p.kind;
    A.tok_s[i] = p.tok_s;
    A.tok_len[i] = p.tok_len;
    A.pos[i] = p.pos;
    A.is_rec[i] = p.kind == K_RECORD;
    if (src == SRC_INFO) {
        uint32_t* c = A.info_cols + 4 * (i - S.line0[2]);
        c[0] = p.c3s; c[1] = p.c3l; c[2] = p.c4s; c[3] = p.c4l;
    }
    if (p.kind == K_RECORD) atomicMax(&st->max_pos, (unsigned long long)p.pos);
    if (p.kind == K_UNDECIDED) atomicAdd(&st->undecided, 1ull);
    if (p.kind == K_BAD) atomicMin(&st->first_bad, (unsigned long long)i);
}

__device__ __forceinline__ bool same_bytes(const uint8_t* t, uint32_t a, uint32_t b, uint32_t n) {
    for (uint32_t k = 0; k < n; ++k) if (t[a + k] != t[b + k]) return false;
    return true;
}

__global__ __launch_bounds__(256) void k_heads(const uint8_t* __restrict__ text, int64_t L, LineArrays A) {
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= L) return;
    int h = 0;
    if (A.kind[i] == K_RECORD)
        h = i == 0 || A.kind[i - 1] != K_RECORD || A.tok_len[i - 1] != A.tok_len[i] || !same_bytes(text, A.tok_s[i - 1], A.tok_s[i], A.tok_len[i]);
    A.is_head[i] = h;
}

__global__ __launch_bounds__(256) void k_head_list(int64_t L, LineArrays A, const int* __restrict__ head_scan, uint32_t* __restrict__ head_tok) {
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= L || !A.is_head[i]) return;
    head_tok[2 * size_t(head_scan[i])] = A.tok_s[i];
    head_tok[2 * size_t(head_scan[i]) + 1] = A.tok_len[i];
}

__global__ __launch_bounds__(256) void k_keys(int64_t L, LineArrays A, const int* __restrict__ head_scan, const int* __restrict__ rec_scan,
                                              const uint32_t* __restrict__ head_rank, uint64_t* __restrict__ keys, uint32_t* __restrict__ pay) {
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= L || !A.is_rec[i]) return;
    const int h = head_scan[i] + A.is_head[i] - 1;         // the last head at or before this line
    keys[rec_scan[i]] = uint64_t(head_rank[h]) << POS_BITS | uint64_t(A.pos[i]);
    pay[rec_scan[i]] = uint32_t(i);
}

// slot t < n_calls: is call line t a header line; slot n_calls + r: does a run start at sorted position r, and is it emitted
__global__ __launch_bounds__(256) void k_runs(Sources S, const uint8_t* __restrict__ kind, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ pay,
                                              int64_t R, int mode, int switch_genotype, int* __restrict__ flag, uint32_t* __restrict__ run_line,
                                              int64_t* __restrict__ run_info, DevStatus* st) {
    const int64_t t = int64_t(blockIdx.x) * 256 + threadIdx.x, Lc = S.line0[1];
    if (t < Lc) { flag[t] = kind[t] == K_HEADER; return; }
    const int64_t r = t - Lc;
    if (r >= R) return;
    flag[t] = 0;
    if (r > 0 && keys[r - 1] == keys[r]) return;
    RunPick pick = {-1, -1, -1};
    for (int64_t q = r; q < R && keys[q] == keys[r]; ++q) {
        const int64_t line = pay[q];
        const int src = source_of(S, line);
        if (src == SRC_CALLS) pick.call = line; else if (src == SRC_LIST) pick.list = line; else pick.info = line;
    }
    if (pick.list >= 0) atomicAdd(&st->counts[0], 1ull);
    if (pick.call >= 0) atomicAdd(&st->counts[1], 1ull);
    if (pick.list >= 0 && pick.call < 0) atomicAdd(&st->counts[2], 1ull);
    const bool emit = mode == 0 ? pick.list >= 0 : (pick.call >= 0 || pick.list >= 0);
    if (!emit) return;
    flag[t] = 1;
    run_line[r] = uint32_t(pick.call >= 0 ? pick.call : pick.list);
    run_info[r] = pick.call < 0 && switch_genotype ? (pick.info >= 0 ? pick.info : -2) : -1;      // -1: kept; -2: rewritten without info
}

__global__ __launch_bounds__(256) void k_plan(const uint8_t* __restrict__ text, Sources S, LineArrays A, int64_t R, const int* __restrict__ flag,
                                              const int* __restrict__ row_of, const uint32_t* __restrict__ run_line, const int64_t* __restrict__ run_info,
                                              Plan* __restrict__ plans, int* __restrict__ lens, DevStatus* st) {
    const int64_t t = int64_t(blockIdx.x) * 256 + threadIdx.x, Lc = S.line0[1];
    if (t >= Lc + R || !flag[t]) return;
    const int64_t line = t < Lc ? t : run_line[t - Lc], info = t < Lc ? -1 : run_info[t - Lc];
    uint32_t s, raw_e;
    line_span(S, A.start, line, source_of(S, line), &s, &raw_e);
    Plan p;
    if (info == -1) p = plan_kept(s, raw_e);
    else {
        const uint32_t e = raw_e > s && text[raw_e - 1] == '\n' ? raw_e - 1 : raw_e;
        const uint32_t* c = info >= 0 ? A.info_cols + 4 * (info - S.line0[2]) : nullptr;
        p = plan_rewrite(text, s, e, info >= 0, c ? c[0] : 0, c ? c[1] : 0, c ? c[2] : 0, c ? c[3] : 0);
        if (p.undecided) atomicAdd(&st->undecided, 1ull);
    }
    plans[row_of[t]] = p;
    lens[row_of[t]] = int(p.out_len);
}

// one wave per output row
__global__ __launch_bounds__(256) void k_compose(const uint8_t* __restrict__ text, const Plan* __restrict__ plans, const long long* __restrict__ off,
                                                 int64_t rows, uint8_t* __restrict__ out) {
    const int64_t row = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const Plan p = plans[row];
    uint8_t* o = out + off[row];
    for (uint32_t i = lane; i < p.pre_len; i += 64) o[i] = text[p.line_s + i];
    if (!p.rewritten) return;
    const uint32_t ra = ref_at(p), ta = tail_at(p);
    for (uint32_t i = lane; i < p.ref_len; i += 64) o[ra + i] = text[p.ref_s + i];
    for (uint32_t i = lane; i < p.tail_len; i += 64) o[ta + i] = text[p.tail_s + i];
    if (lane == 0) write_small(p, o);
}

// ------------------------------------------------------------------------------------------------ host side, shared
const char* const MAJOR[24] = {"1", "2", "3", "4", "5", "6", "7", "8", "9", "10", "11", "12", "13", "14", "15", "16", "17", "18", "19", "20", "21", "22", "X", "Y"};

struct Interner {                  // rule 6
    std::unordered_map<std::string, uint32_t> rank;
    uint32_t next = 48;
    Interner() {
        for (uint32_t k = 0; k < 24; ++k) { rank[std::string("chr") + MAJOR[k]] = k; rank[MAJOR[k]] = 24 + k; }
    }
    uint32_t of(const uint8_t* t, uint32_t s, uint32_t n) {
        auto it = rank.emplace(std::string(reinterpret_cast<const char*>(t) + s, n), next);
        if (it.second) ++next;
        return it.first->second;
    }
};

inline uint64_t bits_below(uint64_t x) { uint64_t m = 0; while (m < x) m = m << 1 | 1; return m; }      // every bit a value <= x can have

template <class F>
void par_for(int64_t n, int threads, F f) {
    threads = int(std::max<int64_t>(1, std::min<int64_t>(threads, n / 4096)));
    if (threads == 1) { f(int64_t(0), n); return; }
    std::vector<std::thread> th;
    for (int k = 0; k < threads; ++k) th.emplace_back([=] { f(n * k / threads, n * (k + 1) / threads); });
    for (auto& x : th) x.join();
}

struct Combined {
    std::vector<uint8_t> text;
    Sources S;
};

int combine(const uint8_t* const* src, const size_t* len, Combined* c) {
    size_t at = 0;
    for (int k = 0; k < 3; ++k) {
        CTO_REQUIRE(len[k] == 0 || src[k], CTO_EINVAL, "cto_add_back: a null text");
        c->S.base[k] = uint32_t(at);
        c->S.len[k] = uint32_t(len[k]);
        at = align16(at + len[k]) + 16;
        CTO_REQUIRE(at < (size_t(1) << 32) - 2 * LINE_TILE, CTO_EUNSUPPORTED, "cto_add_back: more than 4 GB of text");
    }
    c->text.assign(at, 0);
    for (int k = 0; k < 3; ++k) if (len[k]) memcpy(c->text.data() + c->S.base[k], src[k], len[k]);
    return CTO_OK;
}

void report_bad(const Sources& S, int64_t line, cto_add_back_stats* st) {
    const int src = source_of(S, line);
    st->bad_source = src + 1;
    st->bad_line = line - S.line0[src] + 1;
}

// ------------------------------------------------------------------------------------------------ the host path
int64_t add_back_host(Combined& c, int mode, int switch_genotype, int threads, uint8_t* out, size_t cap, int64_t* counts, cto_add_back_stats* st) {
    const uint8_t* t = c.text.data();
    Sources& S = c.S;
    for (int k = 0; k < 3; ++k)
        for (uint32_t i = 0; i < S.len[k]; ++i) { const uint8_t b = t[S.base[k] + i]; if (b == '\r' || b >= 0x80) { st->non_ascii = 1; return 0; } }
    std::vector<uint32_t> ls, le;                          // absolute [start, raw end) of every line
    S.line0[0] = 0;
    for (int k = 0; k < 3; ++k) {
        const uint32_t b = S.base[k], e = b + S.len[k];
        for (uint32_t i = b; i < e;) {
            const void* nl = memchr(t + i, '\n', e - i);
            const uint32_t j = nl ? uint32_t(static_cast<const uint8_t*>(nl) - t) + 1 : e;
            ls.push_back(i); le.push_back(j);
            i = j;
        }
        S.line0[k + 1] = int64_t(ls.size());
    }
    const int64_t L = S.line0[3], Lc = S.line0[1];
    CTO_REQUIRE(L < (int64_t(1) << 30), CTO_EUNSUPPORTED, "cto_add_back: more than 2^30 lines");
    std::vector<Parsed> P(static_cast<size_t>(L));
    par_for(L, threads, [&](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; ++i) {
            const uint32_t e = le[i] > ls[i] && t[le[i] - 1] == '\n' ? le[i] - 1 : le[i];
            P[i] = source_of(S, i) == SRC_INFO ? parse_info_line(t, ls[i], e) : parse_vcf_line(t, ls[i], e);
        }
    });
    int64_t max_pos = 0, first_bad = -1;
    for (int64_t i = 0; i < L; ++i) {
        if (P[i].kind == K_UNDECIDED) ++st->undecided;
        if (P[i].kind == K_BAD && first_bad < 0) first_bad = i;
        if (P[i].kind == K_RECORD) max_pos = std::max(max_pos, P[i].pos);
    }
    if (first_bad >= 0) { report_bad(S, first_bad, st); return 0; }
    if (st->undecided) return 0;
    Interner in;
    std::vector<uint64_t> keys;
    std::vector<uint32_t> pay;
    uint32_t rank = 0;
    for (int64_t i = 0, prev = -1; i < L; ++i) {
        if (P[i].kind != K_RECORD) continue;
        if (prev < 0 || prev != i - 1 || P[prev].tok_len != P[i].tok_len || memcmp(t + P[prev].tok_s, t + P[i].tok_s, P[i].tok_len))
            rank = in.of(t, P[i].tok_s, P[i].tok_len);
        prev = i;
        keys.push_back(uint64_t(rank) << POS_BITS | uint64_t(P[i].pos));
        pay.push_back(uint32_t(i));
    }
    CTO_REQUIRE(in.next - 1 <= MAX_RANK, CTO_EUNSUPPORTED, "cto_add_back: more than %u contig names", MAX_RANK);
    const int64_t R = int64_t(keys.size());
    sort_pairs_host(keys.data(), pay.data(), R, bits_below(uint64_t(max_pos)) | bits_below(in.next - 1) << POS_BITS);
    std::vector<Plan> plans;
    for (int64_t i = 0; i < Lc; ++i) if (P[i].kind == K_HEADER) plans.push_back(plan_kept(ls[i], le[i]));
    counts[0] = counts[1] = counts[2] = 0;
    for (int64_t r = 0; r < R;) {
        RunPick pick = {-1, -1, -1};
        int64_t q = r;
        for (; q < R && keys[q] == keys[r]; ++q) {
            const int64_t line = pay[q];
            const int src = source_of(S, line);
            if (src == SRC_CALLS) pick.call = line; else if (src == SRC_LIST) pick.list = line; else pick.info = line;
        }
        r = q;
        counts[0] += pick.list >= 0;
        counts[1] += pick.call >= 0;
        counts[2] += pick.list >= 0 && pick.call < 0;
        if (!(mode == 0 ? pick.list >= 0 : (pick.call >= 0 || pick.list >= 0))) continue;
        const int64_t line = pick.call >= 0 ? pick.call : pick.list;
        if (pick.call >= 0 || !switch_genotype) { plans.push_back(plan_kept(ls[line], le[line])); continue; }
        const uint32_t e = le[line] > ls[line] && t[le[line] - 1] == '\n' ? le[line] - 1 : le[line];
        const bool has = pick.info >= 0;
        const Parsed z = has ? P[pick.info] : Parsed{};
        plans.push_back(plan_rewrite(t, ls[line], e, has, z.c3s, z.c3l, z.c4s, z.c4l));
        st->undecided += plans.back().undecided;
    }
    if (st->undecided) return 0;
    const int64_t rows = int64_t(plans.size());
    std::vector<int64_t> off(static_cast<size_t>(rows) + 1, 0);
    for (int64_t i = 0; i < rows; ++i) off[i + 1] = off[i] + plans[i].out_len;
    st->n_rows = rows;
    if (size_t(off[rows]) > cap) return off[rows];
    par_for(rows, threads, [&](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; ++i) {
            const Plan& p = plans[i];
            uint8_t* o = out + off[i];
            memcpy(o, t + p.line_s, p.pre_len);
            if (!p.rewritten) continue;
            if (p.ref_len) memcpy(o + ref_at(p), t + p.ref_s, p.ref_len);
            if (p.tail_len) memcpy(o + tail_at(p), t + p.tail_s, p.tail_len);
            write_small(p, o);
        }
    });
    return off[rows];
}

// ------------------------------------------------------------------------------------------------ the device path
struct AddBackCtx {
    std::mutex mu;
    Event ev0, ev1;
    bool ready = false;
    DevBuf text, status, tiles, tile_base, tile_tmp, tile_tot, start, kind, tok_s, tok_len, pos, info_cols, is_rec, is_head, head_scan, rec_scan,
        head_tok, head_rank, ka, kb, pa, pb, flag, row_of, run_line, run_info, plans, lens, off, out;
    SortScratch sort;
};

#define AB_LAUNCH_OK(what)                                                                      \
    do {                                                                                        \
        const hipError_t le__ = hipGetLastError();                                              \
        CTO_REQUIRE(le__ == hipSuccess, CTO_EHIP, "cto_add_back: %s: %s", what, hipGetErrorString(le__)); \
    } while (0)

inline unsigned blocks_of(int64_t n, int per) { return unsigned(std::max<int64_t>(1, cdiv(n, per))); }

int64_t add_back_device(Combined& c, int mode, int switch_genotype, hipStream_t s, uint8_t* out, size_t cap, int64_t* counts, cto_add_back_stats* st) {
    AddBackCtx& x = process_wide<AddBackCtx>();
    std::lock_guard<std::mutex> lock(x.mu);
    int rc;
    if (!x.ready) {
        if ((rc = x.ev0.create()) || (rc = x.ev1.create())) return rc;
        x.ready = true;
    }
    Sources& S = c.S;
    const size_t T = c.text.size();
    if ((rc = x.text.ensure(T)) || (rc = x.status.ensure(sizeof(DevStatus)))) return rc;
    const uint8_t* d_text = x.text.as<uint8_t>();
    DevStatus* d_st = x.status.as<DevStatus>();
    DevStatus hs = {};
    hs.first_bad = ~0ull;
    CTO_HIP(hipMemcpyAsync(x.text.p, c.text.data(), T, hipMemcpyHostToDevice, s));
    CTO_HIP(hipMemcpyAsync(d_st, &hs, sizeof hs, hipMemcpyHostToDevice, s));
    CTO_HIP(hipEventRecord(x.ev0, s));
    hipLaunchKernelGGL(k_byte_class, dim3(blocks_of(int64_t(T), 4096)), dim3(256), 0, s, d_text, uint32_t(T), d_st);
    // line starts, source by source
    int tiles[3], tile0[4] = {0, 0, 0, 0};
    for (int k = 0; k < 3; ++k) { tiles[k] = int(cdiv(int64_t(S.len[k]), LINE_TILE)); tile0[k + 1] = tile0[k] + tiles[k] + 1; }
    if ((rc = x.tiles.ensure(size_t(tile0[3]) * sizeof(int))) || (rc = x.tile_base.ensure(size_t(tile0[3]) * sizeof(int))) ||
        (rc = x.tile_tmp.ensure((T / LINE_TILE / SCAN_TILE + 8) * sizeof(long long))) || (rc = x.tile_tot.ensure(sizeof(long long))))
        return rc;
    for (int k = 0; k < 3; ++k) {
        if (!tiles[k]) continue;
        hipLaunchKernelGGL(k_line_count, dim3(unsigned(tiles[k])), dim3(1024), 0, s, d_text + S.base[k], S.len[k], 0, x.tiles.as<int>() + tile0[k]);
        scan_exclusive<int>(s, x.tiles.as<int>() + tile0[k], tiles[k], x.tile_base.as<int>() + tile0[k], nullptr, x.tile_tmp.as<long long>(),
                            x.tile_tot.as<long long>());
    }
    AB_LAUNCH_OK("line counts");
    S.line0[0] = 0;
    for (int k = 0; k < 3; ++k) {
        int n = 0;
        if (tiles[k]) CTO_HIP(hipMemcpyAsync(&n, x.tile_base.as<int>() + tile0[k] + tiles[k], sizeof n, hipMemcpyDeviceToHost, s));
        CTO_HIP(hipStreamSynchronize(s));
        S.line0[k + 1] = S.line0[k] + n;
    }
    CTO_HIP(hipMemcpyAsync(&hs, d_st, sizeof hs, hipMemcpyDeviceToHost, s));
    CTO_HIP(hipStreamSynchronize(s));
    if (hs.non_ascii) { st->non_ascii = 1; return 0; }
    const int64_t L = S.line0[3], Lc = S.line0[1], Li = L - S.line0[2];
    CTO_REQUIRE(L < (int64_t(1) << 30), CTO_EUNSUPPORTED, "cto_add_back: more than 2^30 lines");
    const size_t Lz = size_t(L) + 1;
    if ((rc = x.start.ensure(Lz * 4)) || (rc = x.kind.ensure(Lz)) || (rc = x.tok_s.ensure(Lz * 4)) || (rc = x.tok_len.ensure(Lz * 4)) ||
        (rc = x.pos.ensure(Lz * 8)) || (rc = x.info_cols.ensure((size_t(Li) + 1) * 16)) || (rc = x.is_rec.ensure(Lz * 4)) ||
        (rc = x.is_head.ensure(Lz * 4)) || (rc = x.head_scan.ensure(Lz * 4)) || (rc = x.rec_scan.ensure(Lz * 4)) ||
        (rc = x.tile_tmp.ensure((Lz / SCAN_TILE + 8) * sizeof(long long))))
        return rc;
    LineArrays A = {x.start.as<uint32_t>(), x.kind.as<uint8_t>(), x.tok_s.as<uint32_t>(), x.tok_len.as<uint32_t>(), x.pos.as<int64_t>(),
                    x.info_cols.as<uint32_t>(), x.is_rec.as<int>(), x.is_head.as<int>()};
    for (int k = 0; k < 3; ++k)
        if (tiles[k])
            hipLaunchKernelGGL(k_line_emit, dim3(unsigned(tiles[k])), dim3(1024), 0, s, d_text + S.base[k], S.len[k], 0, x.tile_base.as<int>() + tile0[k],
                               A.start + S.line0[k]);
    int n_heads = 0, n_rec = 0;
    if (L) {
        hipLaunchKernelGGL(k_parse, dim3(blocks_of(L, 256)), dim3(256), 0, s, d_text, S, A, d_st);
        hipLaunchKernelGGL(k_heads, dim3(blocks_of(L, 256)), dim3(256), 0, s, d_text, L, A);
        scan_exclusive<int>(s, A.is_head, int(L), x.head_scan.as<int>(), nullptr, x.tile_tmp.as<long long>(), x.tile_tot.as<long long>());
        scan_exclusive<int>(s, A.is_rec, int(L), x.rec_scan.as<int>(), nullptr, x.tile_tmp.as<long long>(), x.tile_tot.as<long long>());
        AB_LAUNCH_OK("parse");
        CTO_HIP(hipMemcpyAsync(&n_heads, x.head_scan.as<int>() + L, sizeof(int), hipMemcpyDeviceToHost, s));
        CTO_HIP(hipMemcpyAsync(&n_rec, x.rec_scan.as<int>() + L, sizeof(int), hipMemcpyDeviceToHost, s));
        CTO_HIP(hipMemcpyAsync(&hs, d_st, sizeof hs, hipMemcpyDeviceToHost, s));
        CTO_HIP(hipStreamSynchronize(s));
    }
    if (hs.first_bad != ~0ull) { report_bad(S, int64_t(hs.first_bad), st); return 0; }
    if (hs.undecided) { st->undecided = int64_t(hs.undecided); return 0; }
    const int64_t R = n_rec;
    // contig ranks: the run heads' strings, interned on the host
    std::vector<uint32_t> head_tok(size_t(n_heads) * 2), head_rank(static_cast<size_t>(n_heads));
    Interner in;
    if (n_heads) {
        if ((rc = x.head_tok.ensure(head_tok.size() * 4)) || (rc = x.head_rank.ensure(head_rank.size() * 4))) return rc;
        hipLaunchKernelGGL(k_head_list, dim3(blocks_of(L, 256)), dim3(256), 0, s, L, A, x.head_scan.as<int>(), x.head_tok.as<uint32_t>());
        AB_LAUNCH_OK("heads");
        CTO_HIP(hipMemcpyAsync(head_tok.data(), x.head_tok.p, head_tok.size() * 4, hipMemcpyDeviceToHost, s));
        CTO_HIP(hipStreamSynchronize(s));
        for (int h = 0; h < n_heads; ++h) {
            CTO_REQUIRE(size_t(head_tok[2 * h]) + head_tok[2 * h + 1] <= T, CTO_EHIP, "cto_add_back: a contig token outside the text");
            head_rank[h] = in.of(c.text.data(), head_tok[2 * h], head_tok[2 * h + 1]);
        }
        CTO_REQUIRE(in.next - 1 <= MAX_RANK, CTO_EUNSUPPORTED, "cto_add_back: more than %u contig names", MAX_RANK);
        CTO_HIP(hipMemcpyAsync(x.head_rank.p, head_rank.data(), head_rank.size() * 4, hipMemcpyHostToDevice, s));
    }
    const size_t Rz = size_t(R) + 1, slots = size_t(Lc + R) + 1;
    if ((rc = x.ka.ensure(Rz * 8)) || (rc = x.kb.ensure(Rz * 8)) || (rc = x.pa.ensure(Rz * 4)) || (rc = x.pb.ensure(Rz * 4)) ||
        (rc = x.flag.ensure(slots * 4)) || (rc = x.row_of.ensure(slots * 4)) || (rc = x.run_line.ensure(Rz * 4)) || (rc = x.run_info.ensure(Rz * 8)) ||
        (rc = x.tile_tmp.ensure((slots / SCAN_TILE + 8) * sizeof(long long))))
        return rc;
    int in_b = 0;
    if (R) {
        hipLaunchKernelGGL(k_keys, dim3(blocks_of(L, 256)), dim3(256), 0, s, L, A, x.head_scan.as<int>(), x.rec_scan.as<int>(), x.head_rank.as<uint32_t>(),
                           x.ka.as<uint64_t>(), x.pa.as<uint32_t>());
        const uint64_t varying = bits_below(hs.max_pos) | bits_below(in.next - 1) << POS_BITS;
        if ((rc = sort_pairs_device(s, x.ka.as<uint64_t>(), x.pa.as<uint32_t>(), x.kb.as<uint64_t>(), x.pb.as<uint32_t>(), R, varying, x.sort, &in_b)))
            return rc;
    }
    const uint64_t* sk = in_b ? x.kb.as<uint64_t>() : x.ka.as<uint64_t>();
    const uint32_t* sp = in_b ? x.pb.as<uint32_t>() : x.pa.as<uint32_t>();
    int rows = 0;
    long long total = 0;
    if (Lc + R) {
        hipLaunchKernelGGL(k_runs, dim3(blocks_of(Lc + R, 256)), dim3(256), 0, s, S, A.kind, sk, sp, R, mode, switch_genotype, x.flag.as<int>(),
                           x.run_line.as<uint32_t>(), x.run_info.as<int64_t>(), d_st);
        scan_exclusive<int>(s, x.flag.as<int>(), int(Lc + R), x.row_of.as<int>(), nullptr, x.tile_tmp.as<long long>(), x.tile_tot.as<long long>());
        AB_LAUNCH_OK("runs");
        CTO_HIP(hipMemcpyAsync(&rows, x.row_of.as<int>() + (Lc + R), sizeof(int), hipMemcpyDeviceToHost, s));
        CTO_HIP(hipStreamSynchronize(s));
    }
    if (rows) {
        if ((rc = x.plans.ensure(size_t(rows) * sizeof(Plan))) || (rc = x.lens.ensure((size_t(rows) + 1) * 4)) ||
            (rc = x.off.ensure((size_t(rows) + 1) * sizeof(long long))) || (rc = x.tile_tmp.ensure((size_t(rows) / SCAN_TILE + 8) * sizeof(long long))))
            return rc;
        hipLaunchKernelGGL(k_plan, dim3(blocks_of(Lc + R, 256)), dim3(256), 0, s, d_text, S, A, R, x.flag.as<int>(), x.row_of.as<int>(),
                           x.run_line.as<uint32_t>(), x.run_info.as<int64_t>(), x.plans.as<Plan>(), x.lens.as<int>(), d_st);
        scan_exclusive<long long>(s, x.lens.as<int>(), rows, x.off.as<long long>(), nullptr, x.tile_tmp.as<long long>(), x.tile_tot.as<long long>());
        AB_LAUNCH_OK("plan");
        CTO_HIP(hipMemcpyAsync(&total, x.off.as<long long>() + rows, sizeof total, hipMemcpyDeviceToHost, s));
    }
    CTO_HIP(hipMemcpyAsync(&hs, d_st, sizeof hs, hipMemcpyDeviceToHost, s));
    CTO_HIP(hipStreamSynchronize(s));
    for (int k = 0; k < 3; ++k) counts[k] = int64_t(hs.counts[k]);
    if (hs.undecided) { st->undecided = int64_t(hs.undecided); return 0; }
    st->n_rows = rows;
    if (size_t(total) > cap || !total) {
        CTO_HIP(hipEventRecord(x.ev1, s));
        return total;
    }
    if ((rc = x.out.ensure(size_t(total)))) return rc;
    hipLaunchKernelGGL(k_compose, dim3(blocks_of(rows, 4)), dim3(256), 0, s, d_text, x.plans.as<Plan>(), x.off.as<long long>(), int64_t(rows),
                       x.out.as<uint8_t>());
    AB_LAUNCH_OK("compose");
    CTO_HIP(hipEventRecord(x.ev1, s));
    CTO_HIP(hipMemcpyAsync(out, x.out.p, size_t(total), hipMemcpyDeviceToHost, s));
    CTO_HIP(hipStreamSynchronize(s));
    float ms = 0;
    CTO_HIP(hipEventElapsedTime(&ms, x.ev0, x.ev1));
    st->kernel_ms = ms;
    return total;
}

struct SortCtx {
    std::mutex mu;
    DevBuf ka, kb, pa, pb;
    SortScratch sort;
};

}  // namespace

extern "C" int64_t cto_add_back(const uint8_t* calls, size_t n_calls, const uint8_t* list, size_t n_list, const uint8_t* info, size_t n_info, int mode,
                                int switch_genotype, int where, int host_threads, void* stream, uint8_t* out, size_t cap, int64_t* counts,
                                cto_add_back_stats* stats) try {
    CTO_REQUIRE(counts && stats && (out || !cap), CTO_EINVAL, "cto_add_back: a null pointer");
    CTO_REQUIRE((mode == 0 || mode == 1) && (where == 0 || where == 1), CTO_EINVAL, "cto_add_back: mode and where are 0 or 1");
    *stats = cto_add_back_stats{};
    counts[0] = counts[1] = counts[2] = 0;
    Combined c;
    const uint8_t* src[3] = {calls, list, info};
    const size_t len[3] = {n_calls, n_list, n_info};
    int rc;
    if ((rc = combine(src, len, &c))) return rc;
    stats->host_path = where;
    const int64_t n = where == 1 ? add_back_host(c, mode, switch_genotype != 0, host_threads > 0 ? host_threads : 16, out, cap, counts, stats)
                                 : add_back_device(c, mode, switch_genotype != 0, static_cast<hipStream_t>(stream), out, cap, counts, stats);
    for (int k = 0; k < 3; ++k) stats->n_lines[k] = c.S.line0[k + 1] - c.S.line0[k];
    return n;
} CTO_CATCH("cto_add_back", int64_t)

extern "C" int cto_sort_u64(uint64_t* keys, uint32_t* payload, int64_t n, int where, void* stream) try {
    CTO_REQUIRE(n >= 0 && (n == 0 || (keys && payload)) && (where == 0 || where == 1), CTO_EINVAL, "cto_sort_u64: a null pointer, n < 0 or another `where`");
    CTO_REQUIRE(n <= SORT_MAX_N, CTO_EUNSUPPORTED, "cto_sort_u64: more than 2^30 pairs");
    const uint64_t varying = varying_bits(keys, n);
    if (where == 1) { sort_pairs_host(keys, payload, n, varying); return CTO_OK; }
    if (n < 2) return CTO_OK;
    SortCtx& x = process_wide<SortCtx>();
    std::lock_guard<std::mutex> lock(x.mu);
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc, in_b = 0;
    if ((rc = x.ka.ensure(size_t(n) * 8)) || (rc = x.kb.ensure(size_t(n) * 8)) || (rc = x.pa.ensure(size_t(n) * 4)) || (rc = x.pb.ensure(size_t(n) * 4))) return rc;
    CTO_HIP(hipMemcpyAsync(x.ka.p, keys, size_t(n) * 8, hipMemcpyHostToDevice, s));
    CTO_HIP(hipMemcpyAsync(x.pa.p, payload, size_t(n) * 4, hipMemcpyHostToDevice, s));
    if ((rc = sort_pairs_device(s, x.ka.as<uint64_t>(), x.pa.as<uint32_t>(), x.kb.as<uint64_t>(), x.pb.as<uint32_t>(), n, varying, x.sort, &in_b))) return rc;
    const hipError_t le = hipGetLastError();
    CTO_REQUIRE(le == hipSuccess, CTO_EHIP, "cto_sort_u64: %s", hipGetErrorString(le));
    CTO_HIP(hipMemcpyAsync(keys, in_b ? x.kb.p : x.ka.p, size_t(n) * 8, hipMemcpyDeviceToHost, s));
    CTO_HIP(hipMemcpyAsync(payload, in_b ? x.pb.p : x.pa.p, size_t(n) * 4, hipMemcpyDeviceToHost, s));
    CTO_HIP(hipStreamSynchronize(s));
    return CTO_OK;
} CTO_CATCH("cto_sort_u64", int)
