// Short-read post-calling filters (src/postfilter_variants.py of the reference): the packer of one mpileup job's
// eight-column text, the kernel that evaluates every read-base of every call's +-flanking window, and the host evaluation of the windows
// the kernel declines.  Compiled with -ffp-contract=off: the thresholds of :332-338 and :409 are double multiplies followed by compares.
#include <algorithm>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <unordered_map>
#include <vector>
#include "hip_buffers.h"

namespace {

using namespace cto;

constexpr uint32_t TM_EQ_REF = 1u, TM_HASH_STAR = 2u;          // tok_meta bits; bits 8.. = the insertion's share of ins_length
constexpr int PF_THREADS = 256, PF_WAVES = PF_THREADS / 64;
constexpr int PF_MAX_TOKENS = 64;                              // distinct tokens of a column the kernel counts (one per lane)
constexpr int PF_WORDS = CTO_PF_ID_RANGE / 32;
constexpr int PF_OUT = 10;

struct PfJob {
    int flanking = 0;
    std::vector<int32_t> col_pos;
    std::vector<int64_t> col_off{0};
    std::vector<uint32_t> ent_tok, ent_rid;
    std::vector<int64_t> col_tok_off{0};
    std::vector<uint32_t> tok_cnt, tok_meta;
    std::vector<uint8_t> col_flags;
    std::vector<uint32_t> col_rid_min, col_rid_max;            // over the column's names (min > max: none)
    std::vector<std::string> keys, tokens;
};

// ------------------------------------------------------------------------------------------------ packer
// One row: get_base_list (:147-179) over field 4, the names of field 7 (:245-251), appended to J as one column.
int pack_row(PfJob& J, std::unordered_map<std::string, uint32_t>& intern, int32_t pos, const char* s, size_t n, const char* names, size_t names_len,
             char ref_base) {
    struct Ent { char base; std::string indel; };
    std::vector<Ent> bl;
    std::set<long> starts, ends;
    size_t i = 0;
    while (i < n) {
        const char c = s[i];
        if (c == '+' || c == '-') {
            ++i;
            size_t adv = 0;
            while (i < n && s[i] >= '0' && s[i] <= '9') adv = adv * 10 + size_t(s[i++] - '0');
            CTO_REQUIRE(!bl.empty() && i < n, CTO_EINVAL, "cto_postfilter_pack: POS %d: an indel with no base before it or no sequence after it", pos);
            bl.back().indel = std::string(1, c) + std::string(s + i, std::min(adv, n - i));
            i += adv - 1;                                       // (adv == 0 steps back onto the last digit, as :167 does)
        } else if (c && strchr("ACGTNacgtn#*", c)) {
            bl.push_back({c, std::string()});
        } else if (c == '^') {
            ++i;                                                // the mapping-quality character
            starts.insert(long(bl.size()) - 1);                 // the entry BEFORE the '^' (:173); -1 at the start of a row
        }
        if (c == '$') ends.insert(long(bl.size()) - 1);
        ++i;
    }
    const std::set<long>& rse = starts.size() > ends.size() ? starts : ends;      // :177, the end set on a tie

    std::vector<std::string> nm;
    for (size_t a = 0;;) {                                      // str.split(','): one name more than commas
        const char* q = static_cast<const char*>(memchr(names + a, ',', names_len - a));
        const size_t b = q ? size_t(q - names) : names_len;
        nm.emplace_back(names + a, b - a);
        if (!q) break;
        a = b + 1;
    }
    CTO_REQUIRE(nm.size() >= bl.size(), CTO_EINVAL, "cto_postfilter_pack: POS %d: %zu bases for %zu read names (the reference raises here)", pos,
                bl.size(), nm.size());
    const size_t n_ent = bl.size(), n_names = nm.size();
    const size_t e0 = J.ent_tok.size(), t0 = J.tok_cnt.size();
    uint32_t rmin = 0xffffffffu, rmax = 0;
    std::unordered_map<uint32_t, size_t> last;                  // key -> its last entry of this column
    for (size_t k = 0; k < n_names; ++k) {
        uint32_t word = 0;
        std::string key = nm[k];
        if (k < n_ent) {
            const char b = bl[k].base;
            key += (b == '#' || (b >= 'a' && b <= 'z')) ? "_1" : "_0";
            std::string tok(1, b);
            tok += bl[k].indel;
            for (char& ch : tok) ch = char(toupper(static_cast<unsigned char>(ch)));
            size_t t = t0;
            while (t < J.tok_cnt.size() && J.tokens[t] != tok) ++t;
            if (t == J.tok_cnt.size()) {
                uint32_t meta = 0;
                if (tok.size() == 1 && tok[0] == ref_base) meta |= TM_EQ_REF;
                if (tok == "#" || tok == "*") meta |= TM_HASH_STAR;
                const std::string& ind = bl[k].indel;
                if (ind.size() > 3 && ind[0] == '+') meta |= uint32_t(std::min<size_t>(ind.size() - 1, size_t(2) * size_t(J.flanking))) << 8;
                J.tokens.push_back(tok);
                J.tok_cnt.push_back(0);
                J.tok_meta.push_back(meta);
            }
            CTO_REQUIRE(t - t0 <= CTO_PF_TOKEN_MASK, CTO_EINVAL, "cto_postfilter_pack: POS %d: too many distinct tokens", pos);
            ++J.tok_cnt[t];
            word = uint32_t(t - t0);
        } else {
            word = CTO_PF_EXTRA;
        }
        if (!key.empty() && key.back() == '0') word |= CTO_PF_ENDS0;
        if (!key.empty() && key.back() == '1') word |= CTO_PF_ENDS1;
        auto it = intern.find(key);
        if (it == intern.end()) {
            it = intern.emplace(key, uint32_t(J.keys.size())).first;
            J.keys.push_back(key);
        }
        const uint32_t rid = it->second;
        if (k < n_ent) {
            auto l = last.find(rid);
            if (l != last.end()) J.ent_tok[e0 + l->second] |= CTO_PF_SUPERSEDED;
            last[rid] = k;
        }
        rmin = std::min(rmin, rid);
        rmax = std::max(rmax, rid);
        J.ent_tok.push_back(word);
        J.ent_rid.push_back(rid);
    }
    for (long idx : rse) {                                      // read_name_list[r_idx] (:411), Python indexing
        const long k = idx < 0 ? long(n_names) + idx : idx;
        if (k >= 0 && k < long(n_names)) J.ent_tok[e0 + size_t(k)] |= CTO_PF_RSE;
    }
    J.col_pos.push_back(pos);
    J.col_off.push_back(int64_t(J.ent_tok.size()));
    J.col_tok_off.push_back(int64_t(J.tok_cnt.size()));
    J.col_flags.push_back(double(rse.size()) >= double(n_ent) * 0.2 ? 1 : 0);     // :409, eps_rse
    J.col_rid_min.push_back(rmin);
    J.col_rid_max.push_back(rmax);
    return CTO_OK;
}

// ------------------------------------------------------------------------------------------------ kernel
// The kernel keeps a column's token counts one token per lane and shifts alt_mask by the token index: both need every column of the window
// to have at most PF_MAX_TOKENS (64) distinct tokens.  cto_postfilter_windows is the only place that builds a PfCall and sends such
// windows to the host code instead; a new caller of the kernel must keep that gate.
struct PfCall {
    uint32_t col_lo, col_hi;          // the window's columns in the batch's column arrays, [lo, hi)
    int32_t  centre;                  // the call's own column, -1 when the text has none
    uint32_t rid_min;                 // smallest read id of the window (ids are per job)
    uint64_t alt_mask;                // bit t: token t of the centre column is the alt allele (:424-434, decided per distinct token on the host)
};

__device__ inline uint32_t wave_max(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, uint32_t(__shfl_xor(int(v), o)));
    return v;
}

// One workgroup per call.  LDS: the alt read set A and the union S of the qualifying columns' start/end names as bitsets over
// (read id - rid_min); the host only sends windows whose id range fits.  Waves take columns; a column's per-token count among A's unique,
// non-reference, non-'#'/'*' entries is kept one token per lane (the host only sends windows whose columns have <= 64 tokens).
// A tie for the top count implies top <= |A| / 2 (the tied tokens belong to disjoint keys of A), and such a column is skipped before the
// identity of the top token is used (:332-334): the result does not depend on the order Python's Counter / sorted would list them in.
__global__ __launch_bounds__(PF_THREADS) void k_postfilter_windows(const PfCall* __restrict__ calls, const uint32_t* __restrict__ col_off,
                                                                   const uint32_t* __restrict__ col_tok_off, const uint8_t* __restrict__ col_flags,
                                                                   const uint32_t* __restrict__ ent_tok, const uint32_t* __restrict__ ent_rid,
                                                                   const uint32_t* __restrict__ tok_cnt, const uint32_t* __restrict__ tok_meta,
                                                                   long long* __restrict__ out) {
    __shared__ uint32_t sA[PF_WORDS], sS[PF_WORDS];
    __shared__ uint32_t sAcc[8];                               // |A|, a0, a1, depth, forward, reverse, match_count, |A & S|
    __shared__ unsigned long long sIns;
    const PfCall c = calls[blockIdx.x];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int w = tid; w < PF_WORDS; w += PF_THREADS) { sA[w] = 0; sS[w] = 0; }
    if (tid < 8) sAcc[tid] = 0;
    if (tid == 0) sIns = 0;
    __syncthreads();

    if (c.centre >= 0) {                                       // :416-441
        const uint32_t e0 = col_off[c.centre], e1 = col_off[c.centre + 1];
        uint32_t depth = 0, fwd = 0, rev = 0, nA = 0, a0 = 0, a1 = 0;
        for (uint32_t e = e0 + tid; e < e1; e += PF_THREADS) {
            const uint32_t t = ent_tok[e];
            ++depth;                                           // every name counts, repeated keys too
            fwd += (t & CTO_PF_ENDS0) ? 1 : 0;
            rev += (t & CTO_PF_ENDS1) ? 1 : 0;
            if (!(t & CTO_PF_EXTRA) && ((c.alt_mask >> (t & 63)) & 1)) {
                const uint32_t id = ent_rid[e] - c.rid_min, bit = 1u << (id & 31);
                if (!(atomicOr(&sA[id >> 5], bit) & bit)) {    // a key enters the set once
                    ++nA;
                    a0 += (t & CTO_PF_ENDS0) ? 1 : 0;
                    a1 += (t & CTO_PF_ENDS1) ? 1 : 0;
                }
            }
        }
        if (nA) { atomicAdd(&sAcc[0], nA); atomicAdd(&sAcc[1], a0); atomicAdd(&sAcc[2], a1); }
        if (depth) { atomicAdd(&sAcc[3], depth); atomicAdd(&sAcc[4], fwd); atomicAdd(&sAcc[5], rev); }
    }
    __syncthreads();
    const uint32_t nA = sAcc[0];

    uint32_t match = 0;
    unsigned long long ins = 0;
    for (uint32_t col = c.col_lo + wave; col < c.col_hi; col += PF_WAVES) {
        const uint32_t e0 = col_off[col], e1 = col_off[col + 1], t0 = col_tok_off[col];
        const bool qualifies = col_flags[col] & 1, centre = int32_t(col) == c.centre;
        uint32_t cnt = 0;                                      // lane t: entries of A with token t
        for (uint32_t base = e0; base < e1; base += 64) {
            const uint32_t e = base + lane;
            bool hit = false;
            uint32_t tk = 0;
            if (e < e1) {
                const uint32_t t = ent_tok[e], id = ent_rid[e] - c.rid_min;
                if (qualifies && (t & CTO_PF_RSE)) atomicOr(&sS[id >> 5], 1u << (id & 31));
                if (!centre && !(t & (CTO_PF_SUPERSEDED | CTO_PF_EXTRA))) {
                    tk = t & CTO_PF_TOKEN_MASK;
                    const uint32_t m = tok_meta[t0 + tk];
                    ins += m >> 8;
                    hit = !(m & (TM_EQ_REF | TM_HASH_STAR)) && ((sA[id >> 5] >> (id & 31)) & 1);
                }
            }
            unsigned long long pending = __ballot(hit);
            while (pending) {                                  // one round per distinct token among this batch's hits (usually one)
                const uint32_t lead_tk = uint32_t(__shfl(int(tk), __ffsll((long long)pending) - 1));
                const unsigned long long same = __ballot(hit && tk == lead_tk);
                if (uint32_t(lane) == lead_tk) cnt += uint32_t(__popcll(same));
                pending &= ~same;
            }
        }
        if (centre) continue;                                  // :305-306
        const uint32_t top = wave_max(cnt);
        if (top == 0) continue;                                // len(alt_list) == 0
        const int which = __ffsll((long long)__ballot(cnt == top)) - 1;
        if (lane == 0) {
            const double dA = double(nA), dtop = double(top);
            if (!(dtop >= dA * 1.5) && !(dtop <= dA * 0.5) && !(double(tok_cnt[t0 + which]) >= dtop * 1.5)) ++match;      // :330-341
        }
    }
    if (match) atomicAdd(&sAcc[6], match);
    if (ins) atomicAdd(&sIns, ins);
    __syncthreads();
    uint32_t inter = 0;
    for (int w = tid; w < PF_WORDS; w += PF_THREADS) inter += uint32_t(__popc(sA[w] & sS[w]));
    if (inter) atomicAdd(&sAcc[7], inter);
    __syncthreads();
    if (tid == 0) {
        long long* o = out + size_t(blockIdx.x) * PF_OUT;
        o[0] = sAcc[0];
        o[1] = sAcc[7];
        o[2] = sAcc[6];
        o[3] = (long long)sIns;
        o[4] = sAcc[3];
        o[5] = sAcc[1];
        o[6] = (long long)sAcc[4] - sAcc[1];
        o[7] = sAcc[2];
        o[8] = (long long)sAcc[5] - sAcc[2];
        o[9] = 0;
    }
}

// ------------------------------------------------------------------------------------------------ host evaluation of a declined window
void window_on_host(const PfJob& J, size_t col_lo, size_t col_hi, long centre, uint32_t rid_min, uint32_t rid_max,
                    const std::vector<uint8_t>& alt_tok, int64_t* o) {
    const size_t range = col_hi > col_lo && rid_max >= rid_min ? size_t(rid_max - rid_min) + 1 : 1;
    std::vector<uint8_t> A(range, 0), S(range, 0);
    int64_t nA = 0, a0 = 0, a1 = 0, depth = 0, fwd = 0, rev = 0, match = 0, ins = 0;
    if (centre >= 0) {
        for (int64_t e = J.col_off[centre]; e < J.col_off[centre + 1]; ++e) {
            const uint32_t t = J.ent_tok[e];
            ++depth;
            fwd += (t & CTO_PF_ENDS0) ? 1 : 0;
            rev += (t & CTO_PF_ENDS1) ? 1 : 0;
            if (!(t & CTO_PF_EXTRA) && alt_tok[t & CTO_PF_TOKEN_MASK] && !A[J.ent_rid[e] - rid_min]) {
                A[J.ent_rid[e] - rid_min] = 1;
                ++nA;
                a0 += (t & CTO_PF_ENDS0) ? 1 : 0;
                a1 += (t & CTO_PF_ENDS1) ? 1 : 0;
            }
        }
    }
    std::vector<uint32_t> cnt;
    for (size_t col = col_lo; col < col_hi; ++col) {
        const int64_t t0 = J.col_tok_off[col], ntok = J.col_tok_off[col + 1] - t0;
        const bool centre_col = long(col) == centre;
        cnt.assign(size_t(ntok), 0);
        for (int64_t e = J.col_off[col]; e < J.col_off[col + 1]; ++e) {
            const uint32_t t = J.ent_tok[e], id = J.ent_rid[e] - rid_min;
            if ((J.col_flags[col] & 1) && (t & CTO_PF_RSE)) S[id] = 1;
            if (centre_col || (t & (CTO_PF_SUPERSEDED | CTO_PF_EXTRA))) continue;
            const uint32_t tk = t & CTO_PF_TOKEN_MASK, m = J.tok_meta[t0 + tk];
            ins += m >> 8;
            if (!(m & (TM_EQ_REF | TM_HASH_STAR)) && A[id]) ++cnt[tk];
        }
        if (centre_col) continue;
        int64_t which = -1;
        for (int64_t t = 0; t < ntok; ++t)
            if (cnt[t] > 0 && (which < 0 || cnt[t] > cnt[which])) which = t;
        if (which < 0) continue;
        const double dA = double(nA), dtop = double(cnt[which]);
        if (!(dtop >= dA * 1.5) && !(dtop <= dA * 0.5) && !(double(J.tok_cnt[t0 + which]) >= dtop * 1.5)) ++match;
    }
    int64_t inter = 0;
    for (size_t k = 0; k < range; ++k) inter += A[k] & S[k];
    o[0] = nA; o[1] = inter; o[2] = match; o[3] = ins; o[4] = depth; o[5] = a0; o[6] = fwd - a0; o[7] = a1; o[8] = rev - a1; o[9] = 1;
}

// is token `tok` of the centre column the call's alt allele (:424-434)
bool token_is_alt(const std::string& tok, int kind, size_t ref_len, const char* alt, size_t alt_len) {
    if (kind == 0) return tok.size() == alt_len && memcmp(tok.data(), alt, alt_len) == 0;
    if (kind == 1) {
        if (tok.find('+') == std::string::npos) return false;
        std::string s;
        for (char ch : tok) if (ch != '+') s += ch;
        return s.size() == alt_len && memcmp(s.data(), alt, alt_len) == 0;
    }
    if (kind == 2) return tok.size() - 1 == ref_len && tok.find('-', 1) != std::string::npos;
    return false;
}

struct PfContext : BatchCtx {};                                // the device side of cto_postfilter_windows, one batch at a time

}  // namespace

extern "C" int cto_postfilter_pack(const char* text, size_t len, const char* ref_seq, int64_t region_lo, size_t ref_len, int flanking, void** job) try {
    CTO_REQUIRE(job && (text || len == 0) && flanking >= 0 && flanking < (1 << 22), CTO_EINVAL, "cto_postfilter_pack: bad arguments");
    std::unique_ptr<PfJob> J(new PfJob);
    J->flanking = flanking;
    std::unordered_map<std::string, uint32_t> intern;
    size_t a = 0;
    while (a < len) {
        const char* nl = static_cast<const char*>(memchr(text + a, '\n', len - a));
        const size_t b = nl ? size_t(nl - text) + 1 : len;       // the row with its '\n', as the reference's iteration over stdout yields it
        size_t tabs[8], nt = 0;
        for (size_t k = a; k < b && nt < 8; ++k)
            if (text[k] == '\t') tabs[nt++] = k;
        if (nt >= 7) {                                          // len(columns) >= 8
            const long pos = strtol(text + tabs[0] + 1, nullptr, 10);
            CTO_REQUIRE(J->col_pos.empty() || pos > J->col_pos.back(), CTO_EINVAL, "cto_postfilter_pack: rows are not in ascending POS at %ld", pos);
            const size_t names_end = nt == 8 ? tabs[7] : b;
            const int64_t ri = pos - region_lo;
            const char rb = ref_seq && ri >= 0 && size_t(ri) < ref_len ? ref_seq[ri] : '\0';
            const int rc = pack_row(*J, intern, int32_t(pos), text + tabs[3] + 1, tabs[4] - tabs[3] - 1, text + tabs[6] + 1, names_end - tabs[6] - 1, rb);
            if (rc != CTO_OK) return rc;
        }
        a = b;
    }
    *job = J.release();
    return CTO_OK;
}
CTO_CATCH("cto_postfilter_pack", int)

extern "C" int cto_postfilter_view_of(const void* job, cto_pf_view* v) {
    CTO_REQUIRE(job && v, CTO_EINVAL, "cto_postfilter_view_of: null argument");
    const PfJob& J = *static_cast<const PfJob*>(job);
    v->n_cols = int64_t(J.col_pos.size());
    v->n_names = int64_t(J.ent_tok.size());
    v->n_keys = int64_t(J.keys.size());
    v->n_tokens = int64_t(J.tok_cnt.size());
    v->col_pos = J.col_pos.data();
    v->col_off = J.col_off.data();
    v->ent_tok = J.ent_tok.data();
    v->ent_rid = J.ent_rid.data();
    v->col_tok_off = J.col_tok_off.data();
    v->tok_cnt = J.tok_cnt.data();
    v->tok_meta = J.tok_meta.data();
    v->col_flags = J.col_flags.data();
    return CTO_OK;
}

extern "C" int cto_postfilter_key_string(const void* job, int64_t rid, const char** s) {
    const PfJob* J = static_cast<const PfJob*>(job);
    CTO_REQUIRE(J && s && rid >= 0 && size_t(rid) < J->keys.size(), CTO_EINVAL, "cto_postfilter_key_string: bad arguments");
    *s = J->keys[size_t(rid)].c_str();
    return CTO_OK;
}

extern "C" int cto_postfilter_token_string(const void* job, int64_t col, int64_t tok, const char** s) {
    const PfJob* J = static_cast<const PfJob*>(job);
    CTO_REQUIRE(J && s && col >= 0 && size_t(col) < J->col_pos.size() && tok >= 0 && tok < J->col_tok_off[col + 1] - J->col_tok_off[col], CTO_EINVAL,
                "cto_postfilter_token_string: bad arguments");
    *s = J->tokens[size_t(J->col_tok_off[col] + tok)].c_str();
    return CTO_OK;
}

extern "C" void cto_postfilter_free(void* job) { delete static_cast<PfJob*>(job); }

extern "C" int cto_postfilter_windows(int n_jobs, void* const* jobs, int64_t n_calls, const int32_t* call_job, const int32_t* call_pos,
                                      const int32_t* call_kind, const int32_t* call_ref_len, const char* alt_bytes, const int64_t* alt_off,
                                      int max_id_range, int64_t* out, double* kernel_ms) try {
    CTO_REQUIRE(n_jobs >= 0 && n_calls >= 0 && (n_calls == 0 || (jobs && call_job && call_pos && call_kind && call_ref_len && alt_off && out)),
                CTO_EINVAL, "cto_postfilter_windows: bad arguments");
    CTO_REQUIRE(max_id_range >= 0 && max_id_range <= CTO_PF_ID_RANGE, CTO_EINVAL, "cto_postfilter_windows: max_id_range is 0..%d", CTO_PF_ID_RANGE);
    if (kernel_ms) *kernel_ms = 0.0;
    int n_dev = 0;
    CTO_REQUIRE(hipGetDeviceCount(&n_dev) == hipSuccess && n_dev > 0, CTO_EHIP, "cto_postfilter_windows: no HIP device (there is no CPU path)");
    if (n_calls == 0) return CTO_OK;
    const uint32_t id_range = max_id_range ? uint32_t(max_id_range) : uint32_t(CTO_PF_ID_RANGE);

    // where each job's columns, names and tokens start in the batch's arrays
    std::vector<size_t> col_base(size_t(n_jobs) + 1, 0), ent_base(size_t(n_jobs) + 1, 0), tok_base(size_t(n_jobs) + 1, 0);
    for (int j = 0; j < n_jobs; ++j) {
        CTO_REQUIRE(jobs[j], CTO_EINVAL, "cto_postfilter_windows: job %d is null", j);
        const PfJob& J = *static_cast<const PfJob*>(jobs[j]);
        col_base[j + 1] = col_base[j] + J.col_pos.size();
        ent_base[j + 1] = ent_base[j] + J.ent_tok.size();
        tok_base[j + 1] = tok_base[j] + J.tok_cnt.size();
    }
    const size_t n_cols = col_base[n_jobs], n_ent = ent_base[n_jobs], n_tok = tok_base[n_jobs];
    CTO_REQUIRE(n_ent < 0xfffffff0u && n_tok < 0xfffffff0u, CTO_EINVAL, "cto_postfilter_windows: batch too large (%zu names)", n_ent);

    // per call: the window's columns, the alt tokens of its centre column, and whether the kernel takes it
    std::vector<PfCall> dev_calls;
    std::vector<int64_t> dev_index;
    std::vector<uint8_t> alt_tok;
    for (int64_t i = 0; i < n_calls; ++i) {
        const int j = call_job[i];
        CTO_REQUIRE(j >= 0 && j < n_jobs, CTO_EINVAL, "cto_postfilter_windows: call %lld names job %d", (long long)i, j);
        const PfJob& J = *static_cast<const PfJob*>(jobs[j]);
        const int64_t pos = call_pos[i], lo = std::max<int64_t>(pos - J.flanking, 1), hi = pos + J.flanking;
        const size_t c0 = size_t(std::lower_bound(J.col_pos.begin(), J.col_pos.end(), lo) - J.col_pos.begin());
        const size_t c1 = size_t(std::upper_bound(J.col_pos.begin(), J.col_pos.end(), hi) - J.col_pos.begin());
        const size_t cc = size_t(std::lower_bound(J.col_pos.begin(), J.col_pos.end(), pos) - J.col_pos.begin());
        const long centre = cc < J.col_pos.size() && J.col_pos[cc] == pos ? long(cc) : -1;
        uint32_t rmin = 0xffffffffu, rmax = 0;
        int64_t max_tok = 0;
        for (size_t c = c0; c < c1; ++c) {
            if (J.col_rid_min[c] <= J.col_rid_max[c]) { rmin = std::min(rmin, J.col_rid_min[c]); rmax = std::max(rmax, J.col_rid_max[c]); }
            max_tok = std::max(max_tok, J.col_tok_off[c + 1] - J.col_tok_off[c]);
        }
        if (rmin > rmax) rmin = rmax = 0;
        alt_tok.clear();
        uint64_t mask = 0;
        if (centre >= 0) {
            const int64_t t0 = J.col_tok_off[centre], nt = J.col_tok_off[centre + 1] - t0;
            alt_tok.assign(size_t(nt) + 1, 0);
            for (int64_t t = 0; t < nt; ++t) {
                alt_tok[t] = token_is_alt(J.tokens[size_t(t0 + t)], call_kind[i], size_t(call_ref_len[i]), alt_bytes + alt_off[i], size_t(alt_off[i + 1] - alt_off[i]));
                if (alt_tok[t] && t < 64) mask |= uint64_t(1) << t;
            }
        }
        if (rmax - rmin < id_range && max_tok <= PF_MAX_TOKENS) {
            dev_calls.push_back({uint32_t(col_base[j] + c0), uint32_t(col_base[j] + c1), centre >= 0 ? int32_t(col_base[j] + size_t(centre)) : -1, rmin, mask});
            dev_index.push_back(i);
        } else {
            window_on_host(J, c0, c1, centre, rmin, rmax, alt_tok, out + i * PF_OUT);
        }
    }
    if (dev_calls.empty()) return CTO_OK;

    // one upload of the batch: [calls | col_off | col_tok_off | ent_tok | ent_rid | tok_cnt | tok_meta | col_flags]
    const size_t n_dev_calls = dev_calls.size();
    size_t off[9];
    off[0] = 0;
    off[1] = off[0] + align16(n_dev_calls * sizeof(PfCall));
    off[2] = off[1] + align16((n_cols + 1) * 4);
    off[3] = off[2] + align16((n_cols + 1) * 4);
    off[4] = off[3] + align16(n_ent * 4);
    off[5] = off[4] + align16(n_ent * 4);
    off[6] = off[5] + align16(n_tok * 4);
    off[7] = off[6] + align16(n_tok * 4);
    off[8] = off[7] + align16(n_cols + 1);
    PfContext& X = process_wide<PfContext>();
    std::lock_guard<std::mutex> lock(X.mu);
    if (const int rc = X.open(off[8], n_dev_calls * PF_OUT * 8)) return rc;
    char* h = X.h_in.as<char>();
    memcpy(h + off[0], dev_calls.data(), n_dev_calls * sizeof(PfCall));
    uint32_t* h_col_off = reinterpret_cast<uint32_t*>(h + off[1]);
    uint32_t* h_tok_off = reinterpret_cast<uint32_t*>(h + off[2]);
    for (int j = 0; j < n_jobs; ++j) {
        const PfJob& J = *static_cast<const PfJob*>(jobs[j]);
        for (size_t c = 0; c < J.col_pos.size(); ++c) {
            h_col_off[col_base[j] + c] = uint32_t(ent_base[j] + size_t(J.col_off[c]));
            h_tok_off[col_base[j] + c] = uint32_t(tok_base[j] + size_t(J.col_tok_off[c]));
        }
        if (!J.ent_tok.empty()) {
            memcpy(h + off[3] + ent_base[j] * 4, J.ent_tok.data(), J.ent_tok.size() * 4);
            memcpy(h + off[4] + ent_base[j] * 4, J.ent_rid.data(), J.ent_rid.size() * 4);
        }
        if (!J.tok_cnt.empty()) {
            memcpy(h + off[5] + tok_base[j] * 4, J.tok_cnt.data(), J.tok_cnt.size() * 4);
            memcpy(h + off[6] + tok_base[j] * 4, J.tok_meta.data(), J.tok_meta.size() * 4);
        }
        if (!J.col_flags.empty()) memcpy(h + off[7] + col_base[j], J.col_flags.data(), J.col_flags.size());
    }
    h_col_off[n_cols] = uint32_t(n_ent);                        // (a job's last column ends where the next job's first begins)
    h_tok_off[n_cols] = uint32_t(n_tok);
    char* d = X.d_in.as<char>();
    CTO_HIP(hipMemcpyAsync(d, h, off[8], hipMemcpyHostToDevice, X.stream));
    CTO_HIP(hipEventRecord(X.ev0, X.stream));
    hipLaunchKernelGGL(k_postfilter_windows, dim3(uint32_t(n_dev_calls)), dim3(PF_THREADS), 0, X.stream, reinterpret_cast<const PfCall*>(d + off[0]),
                       reinterpret_cast<const uint32_t*>(d + off[1]), reinterpret_cast<const uint32_t*>(d + off[2]),
                       reinterpret_cast<const uint8_t*>(d + off[7]), reinterpret_cast<const uint32_t*>(d + off[3]),
                       reinterpret_cast<const uint32_t*>(d + off[4]), reinterpret_cast<const uint32_t*>(d + off[5]),
                       reinterpret_cast<const uint32_t*>(d + off[6]), X.d_out.as<long long>());
    CTO_HIP(hipGetLastError());
    CTO_HIP(hipEventRecord(X.ev1, X.stream));
    CTO_HIP(hipMemcpyAsync(X.h_out.p, X.d_out.p, n_dev_calls * PF_OUT * 8, hipMemcpyDeviceToHost, X.stream));
    CTO_HIP(record_and_wait(X.done, X.stream));
    if (kernel_ms) {
        float ms = 0.f;
        CTO_HIP(hipEventElapsedTime(&ms, X.ev0, X.ev1));
        *kernel_ms = ms;
    }
    const int64_t* r = X.h_out.as<int64_t>();
    for (size_t k = 0; k < n_dev_calls; ++k) memcpy(out + dev_index[k] * PF_OUT, r + k * PF_OUT, PF_OUT * 8);
    return CTO_OK;
}
CTO_CATCH("cto_postfilter_windows", int)
