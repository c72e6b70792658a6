// BGZF deflate: the rules of csrc/deflate.hip as plain sequential C++ on the standard library alone (the host path of
// cto_bgzf_deflate, and the functions the kernel shares with it: everything marked CTO_HD is compiled for both sides from this one
// text, so the two cannot drift apart).  The rules themselves are written out in the header comment of deflate.hip.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define CTO_HD __host__ __device__ inline
#else
#define CTO_HD inline
#endif

#ifndef CTO_DEFLATE_SEG
#define CTO_DEFLATE_SEG 512            // rule 2: bytes of a segment (tools/deflate_bench.py builds the coder with other values)
#endif
#ifndef CTO_DEFLATE_PROBES
#define CTO_DEFLATE_PROBES 1, 2, 3, 4, 6, 8   // rule 3: the distances tried beside the hash table's candidate
#endif

namespace cto {
namespace dfl {

constexpr int kPayload = 0xff00;       // input bytes of a block (CTO_BGZF_PAYLOAD)
constexpr int kSlot = 65536;           // output bytes reserved per block
constexpr int kSeg = CTO_DEFLATE_SEG;
constexpr int kTile = 256;             // positions that look the table up before any of them enters it
constexpr int kHashBits = 14;
constexpr int kMinMatch = 3, kMaxMatch = 258, kMaxDist = 32768, kFar3 = 4096;
constexpr int kNumLL = 286, kNumD = 30, kNumCL = 19, kHist = kNumLL + kNumD;
constexpr int kMaxPayloadOut = kSlot - 26;

CTO_HD uint32_t hash4(const uint8_t* p) {
    const uint32_t v = uint32_t(p[0]) | (uint32_t(p[1]) << 8) | (uint32_t(p[2]) << 16) | (uint32_t(p[3]) << 24);
    return (v * 2654435761u) >> (32 - kHashBits);
}

// rule 3: the match at p, (length << 16) | distance, or 0.  cand: the table's candidate (-1: none).
CTO_HD uint32_t match_at(const uint8_t* d, int n, int p, int cand) {
    constexpr int probes[] = {CTO_DEFLATE_PROBES};
    constexpr int n_probes = int(sizeof(probes) / sizeof(probes[0]));
    const int seg_end = (p / kSeg + 1) * kSeg < n ? (p / kSeg + 1) * kSeg : n;
    const int max_len = seg_end - p < kMaxMatch ? seg_end - p : kMaxMatch;
    if (max_len < kMinMatch) return 0;
    int best_len = 0, best_dist = 0;
    for (int k = -1; k < n_probes; ++k) {
        const int q = k < 0 ? cand : p - probes[k];
        if (q < 0 || q >= p || p - q > kMaxDist) continue;
        int len = 0;
        while (len < max_len && d[q + len] == d[p + len]) ++len;
        if (len > best_len || (len == best_len && p - q < best_dist)) { best_len = len; best_dist = p - q; }
    }
    if (best_len < kMinMatch || (best_len == kMinMatch && best_dist > kFar3)) return 0;
    return (uint32_t(best_len) << 16) | uint32_t(best_dist);
}

CTO_HD int floor_log2(uint32_t x) { return 31 - __builtin_clz(x); }
// RFC 1951's length and distance codes: symbol, number of extra bits, their value
CTO_HD void length_code(int len, int* sym, int* eb, int* ev) {
    const int l = len - 3;
    if (len == 258) { *sym = 285; *eb = 0; *ev = 0; }
    else if (l < 8) { *sym = 257 + l; *eb = 0; *ev = 0; }
    else { const int e = floor_log2(uint32_t(l)) - 2; *sym = 257 + 4 * (e + 1) + ((l >> e) & 3); *eb = e; *ev = l & ((1 << e) - 1); }
}
CTO_HD void dist_code(int dist, int* sym, int* eb, int* ev) {
    const int d = dist - 1;
    if (d < 4) { *sym = d; *eb = 0; *ev = 0; }
    else { const int hb = floor_log2(uint32_t(d)), e = hb - 1; *sym = 2 * hb + ((d >> e) & 1); *eb = e; *ev = d & ((1 << e) - 1); }
}
CTO_HD int ll_extra_bits(int sym) { return sym < 265 || sym == 285 ? 0 : (sym - 261) >> 2; }
CTO_HD int d_extra_bits(int sym) { return sym < 4 ? 0 : (sym >> 1) - 1; }

// rule 2/4: the tokens of one segment, in order: f(0, byte) for a literal, f(length, distance) for a match
template <class F> CTO_HD void walk_segment(const uint8_t* d, const uint32_t* match, int n, int seg, F&& f) {
    int p = seg * kSeg;
    const int end = p + kSeg < n ? p + kSeg : n;
    while (p < end) {
        const uint32_t m = match[p];
        if (m) { f(int(m >> 16), int(m & 0xffffu)); p += int(m >> 16); }
        else { f(0, int(d[p])); ++p; }
    }
}

// scratch of the code construction and the plan of one block: in LDS on the device, on the stack on the host
struct HuffWs {
    uint32_t f_ll[288], f_d[32];          // the frequencies the codes are built from (the histogram with the forced pair)
    uint16_t ord_ll[288], ord_d[32];      // symbols ascending by (frequency, symbol)
    uint32_t w[2 * 288];
    uint16_t parent[2 * 288];
    int num[48];
};
struct Plan {
    uint8_t ll_len[288], d_len[32], cl_len[kNumCL];        // the dynamic code lengths
    uint8_t e_ll_len[288], e_d_len[32];                    // lengths and codes (bit-reversed) the block is emitted with
    uint16_t e_ll_code[288], e_d_code[32], cl_code[kNumCL];
    uint8_t tok_sym[kHist + 4], tok_ext[kHist + 4];        // the code-length header as symbols 0 .. 18 and their extra value
    int n_tok, hlit, hdist, hclen;
    long long bits[3];                                     // stored, fixed, dynamic
    int type;                                              // 0 stored, 1 fixed, 2 dynamic
};

// rule 5a: fewer than two used symbols: the unused symbols 0, 1, 2 get frequency 1 in turn until two are used
CTO_HD void force_pair(uint32_t* f, int n) {
    int used = 0;
    for (int i = 0; i < n; ++i) used += f[i] != 0;
    for (int i = 0; i < n && i < 3 && used < 2; ++i) if (!f[i]) { f[i] = 1; ++used; }
}
CTO_HD bool freq_less(const uint32_t* f, int a, int b) { return f[a] < f[b] || (f[a] == f[b] && a < b); }
// the order a sort by (frequency, symbol) gives; the kernel ranks the large alphabets in parallel instead
CTO_HD void sort_order(const uint32_t* f, int n, uint16_t* ord) {
    for (int i = 0; i < n; ++i) {
        int j = i;
        for (; j > 0 && freq_less(f, i, ord[j - 1]); --j) ord[j] = ord[j - 1];
        ord[j] = uint16_t(i);
    }
}

// rule 5b: code lengths of at most max_bits for the symbols of non-zero frequency (at least two; ord as sort_order gives it)
CTO_HD void build_lengths(const uint32_t* f, int n, const uint16_t* ord, int max_bits, HuffWs* ws, uint8_t* len) {
    int z = 0;
    while (z < n && f[ord[z]] == 0) ++z;
    const int m = n - z;                                   // used symbols: ord[z .. n)
    for (int i = 0; i < n; ++i) len[i] = 0;
    if (m < 2) { if (m == 1) len[ord[z]] = 1; return; }    // not reached behind force_pair
    uint32_t* w = ws->w;
    uint16_t* parent = ws->parent;
    for (int i = 0; i < m; ++i) w[i] = f[ord[z + i]];
    int i = 0, j = m;                                      // next leaf, next inner node not yet joined
    for (int k = m; k < 2 * m - 1; ++k) {
        uint32_t sum = 0;
        for (int t = 0; t < 2; ++t) {
            const int a = (i < m && (j >= k || w[i] <= w[j])) ? i++ : j++;       // a leaf wins a tie
            parent[a] = uint16_t(k);
            sum += w[a];
        }
        w[k] = sum;
    }
    int* num = ws->num;
    for (int b = 0; b <= max_bits; ++b) num[b] = 0;
    w[2 * m - 2] = 0;                                      // from here: depth
    for (int t = 2 * m - 3; t >= 0; --t) {
        w[t] = w[parent[t]] + 1;
        if (t < m) ++num[w[t] < uint32_t(max_bits) ? int(w[t]) : max_bits];
    }
    uint32_t total = 0;
    for (int b = 1; b <= max_bits; ++b) total += uint32_t(num[b]) << (max_bits - b);
    while (total > (1u << max_bits)) {                     // one leaf of the deepest level up beside a leaf moved one level down
        --num[max_bits];
        for (int b = max_bits - 1; b > 0; --b) if (num[b]) { --num[b]; num[b + 1] += 2; break; }
        --total;
    }
    int at = n;                                            // the most frequent symbols get the shortest codes
    for (int b = 1; b <= max_bits; ++b) for (int c = num[b]; c > 0; --c) len[ord[--at]] = uint8_t(b);
}

// canonical codes of RFC 1951 3.2.2, bit-reversed for a writer that fills bytes from the low bit
CTO_HD void make_codes(const uint8_t* len, int n, uint16_t* code) {
    int count[16], next[16];
    for (int b = 0; b < 16; ++b) count[b] = 0;
    for (int i = 0; i < n; ++i) ++count[len[i]];
    count[0] = 0;
    int c = 0;
    next[0] = 0;
    for (int b = 1; b < 16; ++b) { c = (c + count[b - 1]) << 1; next[b] = c; }
    for (int i = 0; i < n; ++i) {
        const int L = len[i];
        uint32_t v = L ? uint32_t(next[L]++) : 0, r = 0;
        for (int b = 0; b < L; ++b) r |= ((v >> b) & 1u) << (L - 1 - b);
        code[i] = uint16_t(r);
    }
}
CTO_HD int fixed_ll_len(int s) { return s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8; }

// rules 5 and 6 for one block: hist is the token histogram (literal/length 0 .. 285, then distance 0 .. 29); ws->f_* and ws->ord_*
// are filled in.  One lane on the device.
CTO_HD void plan_block(const uint32_t* hist, int n, HuffWs* ws, Plan* pl) {
    build_lengths(ws->f_ll, kNumLL, ws->ord_ll, 15, ws, pl->ll_len);
    build_lengths(ws->f_d, kNumD, ws->ord_d, 15, ws, pl->d_len);
    pl->ll_len[286] = pl->ll_len[287] = 0;
    pl->d_len[30] = pl->d_len[31] = 0;
    int hlit = kNumLL, hdist = kNumD;
    while (hlit > 257 && !pl->ll_len[hlit - 1]) --hlit;
    while (hdist > 1 && !pl->d_len[hdist - 1]) --hdist;
    // rule 5c: the lengths of both alphabets as one sequence, runs folded into the repeat codes
    const int N = hlit + hdist;
    int nt = 0;
    uint32_t cl_f[kNumCL];
    for (int s = 0; s < kNumCL; ++s) cl_f[s] = 0;
    auto emit = [&](int s, int ext) { pl->tok_sym[nt] = uint8_t(s); pl->tok_ext[nt] = uint8_t(ext); ++nt; ++cl_f[s]; };
    for (int i = 0; i < N;) {
        const int v = i < hlit ? pl->ll_len[i] : pl->d_len[i - hlit];
        int run = 1;
        while (i + run < N && (i + run < hlit ? pl->ll_len[i + run] : pl->d_len[i + run - hlit]) == v) ++run;
        i += run;
        if (v) { emit(v, 0); --run; }
        while (run > 0) {
            int r = 1;
            if (v == 0 && run >= 11) { r = run < 138 ? run : 138; emit(18, r - 11); }
            else if (v == 0 && run >= 3) { r = run; emit(17, r - 3); }
            else if (v != 0 && run >= 3) { r = run < 6 ? run : 6; emit(16, r - 3); }
            else emit(v, 0);
            run -= r;
        }
    }
    pl->n_tok = nt;
    pl->hlit = hlit;
    pl->hdist = hdist;
    force_pair(cl_f, kNumCL);
    uint16_t cl_ord[kNumCL];
    sort_order(cl_f, kNumCL, cl_ord);
    build_lengths(cl_f, kNumCL, cl_ord, 7, ws, pl->cl_len);
    make_codes(pl->cl_len, kNumCL, pl->cl_code);
    const int order[kNumCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    int hclen = kNumCL;
    while (hclen > 4 && !pl->cl_len[order[hclen - 1]]) --hclen;
    pl->hclen = hclen;
    // rule 6: the three sizes in bits
    long long fixed = 3, dyn = 3 + 14 + 3 * hclen;
    for (int t = 0; t < nt; ++t) { const int s = pl->tok_sym[t]; dyn += pl->cl_len[s] + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0); }
    for (int s = 0; s < kNumLL; ++s) {
        fixed += (long long)hist[s] * (fixed_ll_len(s) + ll_extra_bits(s));
        dyn += (long long)hist[s] * (pl->ll_len[s] + ll_extra_bits(s));
    }
    for (int s = 0; s < kNumD; ++s) {
        fixed += (long long)hist[kNumLL + s] * (5 + d_extra_bits(s));
        dyn += (long long)hist[kNumLL + s] * (pl->d_len[s] + d_extra_bits(s));
    }
    pl->bits[0] = 8LL * (n + 5);
    pl->bits[1] = fixed;
    pl->bits[2] = dyn;
    int type = 0;
    if (pl->bits[1] < pl->bits[type]) type = 1;
    if (pl->bits[2] < pl->bits[type]) type = 2;
    if ((pl->bits[type] + 7) / 8 > kMaxPayloadOut) type = 0;
    pl->type = type;
    if (type == 1) {
        for (int s = 0; s < 288; ++s) pl->e_ll_len[s] = uint8_t(fixed_ll_len(s));
        for (int s = 0; s < 32; ++s) pl->e_d_len[s] = 5;
    } else {
        for (int s = 0; s < 288; ++s) pl->e_ll_len[s] = pl->ll_len[s];
        for (int s = 0; s < 32; ++s) pl->e_d_len[s] = pl->d_len[s];
    }
    make_codes(pl->e_ll_len, 288, pl->e_ll_code);
    make_codes(pl->e_d_len, 32, pl->e_d_code);
}

// rule 7: `nb` (at most 32) bits of v at bit position *pos of a zeroed array of 32-bit words; or_word(i, x) ORs x into word i
template <class Or> CTO_HD void put_bits(Or&& or_word, uint32_t* pos, uint32_t v, int nb) {
    if (nb) {
        const uint64_t x = uint64_t(v) << (*pos & 31u);
        or_word(*pos >> 5, uint32_t(x));
        if (x >> 32) or_word((*pos >> 5) + 1, uint32_t(x >> 32));
        *pos += uint32_t(nb);
    }
}
// the bits of one token under the plan's codes, and the token written
CTO_HD int token_bits(const Plan* pl, int len, int v) {
    if (!len) return pl->e_ll_len[v];
    int ls, le, lv, ds, de, dv;
    length_code(len, &ls, &le, &lv);
    dist_code(v, &ds, &de, &dv);
    return pl->e_ll_len[ls] + le + pl->e_d_len[ds] + de;
}
template <class Or> CTO_HD void put_token(Or&& or_word, uint32_t* pos, const Plan* pl, int len, int v) {
    if (!len) { put_bits(or_word, pos, pl->e_ll_code[v], pl->e_ll_len[v]); return; }
    int ls, le, lv, ds, de, dv;
    length_code(len, &ls, &le, &lv);
    dist_code(v, &ds, &de, &dv);
    put_bits(or_word, pos, uint32_t(pl->e_ll_code[ls]) | (uint32_t(lv) << pl->e_ll_len[ls]), pl->e_ll_len[ls] + le);
    put_bits(or_word, pos, uint32_t(pl->e_d_code[ds]) | (uint32_t(dv) << pl->e_d_len[ds]), pl->e_d_len[ds] + de);
}
// the block header in front of the first token; returns its bits
template <class Or> CTO_HD uint32_t put_header(Or&& or_word, const Plan* pl) {
    uint32_t pos = 0;
    put_bits(or_word, &pos, 1u | (uint32_t(pl->type) << 1), 3);
    if (pl->type == 2) {
        const int order[kNumCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        put_bits(or_word, &pos, uint32_t(pl->hlit - 257) | (uint32_t(pl->hdist - 1) << 5) | (uint32_t(pl->hclen - 4) << 10), 14);
        for (int k = 0; k < pl->hclen; ++k) put_bits(or_word, &pos, pl->cl_len[order[k]], 3);
        for (int t = 0; t < pl->n_tok; ++t) {
            const int s = pl->tok_sym[t];
            put_bits(or_word, &pos, pl->cl_code[s], pl->cl_len[s]);
            put_bits(or_word, &pos, pl->tok_ext[t], s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0);
        }
    }
    return pos;
}

// the 18 bytes in front of a block's payload and the 8 behind it; total: the whole block's size
CTO_HD void bgzf_frame(uint8_t* out, int clen, uint32_t crc, uint32_t isize) {
    const uint8_t head[16] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0};
    for (int k = 0; k < 16; ++k) out[k] = head[k];
    const uint32_t bs = uint32_t(clen + 25);
    out[16] = uint8_t(bs);
    out[17] = uint8_t(bs >> 8);
    uint8_t* t = out + 18 + clen;
    for (int k = 0; k < 4; ++k) { t[k] = uint8_t(crc >> (8 * k)); t[4 + k] = uint8_t(isize >> (8 * k)); }
}

// ---- the host path: the sequential definition ------------------------------------------------------------------------------

inline uint32_t crc32_host(const uint8_t* p, size_t n) {
    static const std::vector<uint32_t> table = [] {
        std::vector<uint32_t> t(256);
        for (uint32_t i = 0; i < 256; ++i) { uint32_t c = i; for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1; t[i] = c; }
        return t;
    }();
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) c = table[(c ^ p[i]) & 0xFFu] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

// rules 1 .. 3: the match of every position
inline void matches_host(const uint8_t* d, int n, std::vector<uint32_t>* match) {
    match->assign(size_t(n) + 1, 0);
    std::vector<int> table(size_t(1) << kHashBits, -1);
    for (int t0 = 0; t0 < n; t0 += kTile) {
        const int t1 = std::min(n, t0 + kTile);
        for (int p = t0; p < t1; ++p) (*match)[size_t(p)] = match_at(d, n, p, p + 4 <= n ? table[hash4(d + p)] : -1);
        for (int p = t0; p < t1; ++p) if (p + 4 <= n) table[hash4(d + p)] = p;
    }
}

struct BlockInfo { long long bits[3]; int type; uint32_t hist[kHist]; };

// one whole BGZF block of d[0 .. n), n <= 0xff00, into out (65536 bytes of room); returns its size
inline int encode_block(const uint8_t* d, int n, uint8_t* out, BlockInfo* info = nullptr) {
    std::vector<uint32_t> match;
    matches_host(d, n, &match);
    const int n_seg = (n + kSeg - 1) / kSeg;
    uint32_t hist[kHist] = {0};
    for (int s = 0; s < n_seg; ++s)
        walk_segment(d, match.data(), n, s, [&](int len, int v) {
            if (!len) { ++hist[v]; return; }
            int ls, le, lv, ds, de, dv;
            length_code(len, &ls, &le, &lv);
            dist_code(v, &ds, &de, &dv);
            ++hist[ls];
            ++hist[kNumLL + ds];
        });
    ++hist[256];
    HuffWs ws;
    Plan pl;
    for (int s = 0; s < 288; ++s) ws.f_ll[s] = s < kNumLL ? hist[s] : 0;
    for (int s = 0; s < 32; ++s) ws.f_d[s] = s < kNumD ? hist[kNumLL + s] : 0;
    force_pair(ws.f_ll, kNumLL);
    force_pair(ws.f_d, kNumD);
    sort_order(ws.f_ll, kNumLL, ws.ord_ll);
    sort_order(ws.f_d, kNumD, ws.ord_d);
    plan_block(hist, n, &ws, &pl);
    if (info) { for (int k = 0; k < 3; ++k) info->bits[k] = pl.bits[k]; info->type = pl.type; memcpy(info->hist, hist, sizeof hist); }
    uint8_t* pay = out + 18;
    int clen;
    if (pl.type == 0) {
        clen = n + 5;
        pay[0] = 1;
        pay[1] = uint8_t(n); pay[2] = uint8_t(n >> 8); pay[3] = uint8_t(~n); pay[4] = uint8_t((~n) >> 8);
        if (n) memcpy(pay + 5, d, size_t(n));
    } else {
        clen = int((pl.bits[pl.type] + 7) / 8);
        std::vector<uint32_t> words(size_t(clen) / 4 + 3, 0);
        auto or_word = [&](uint32_t i, uint32_t x) { words[i] |= x; };
        uint32_t pos = put_header(or_word, &pl);
        for (int s = 0; s < n_seg; ++s) walk_segment(d, match.data(), n, s, [&](int len, int v) { put_token(or_word, &pos, &pl, len, v); });
        put_bits(or_word, &pos, pl.e_ll_code[256], pl.e_ll_len[256]);
        for (int i = 0; i < clen; ++i) pay[i] = uint8_t(words[size_t(i) >> 2] >> (8 * (i & 3)));
    }
    bgzf_frame(out, clen, crc32_host(d, size_t(n)), uint32_t(n));
    return 18 + clen + 8;
}

}  // namespace dfl
}  // namespace cto
