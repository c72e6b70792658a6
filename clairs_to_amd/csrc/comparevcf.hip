// compare_vcf, the evaluation command of the reference (src/compare_vcf.py:82-538): the input calls and the truth records, both parsed and
// in dict order, are classified into the reference's five key sets and its counters, and the QUAL cut-offs of --output_best_f1_score and
// --roc_fn are counted - the kernels, the host path of the same call, the entry points.  Every output is an integer: the two paths are
// equal.  DESIGN.md "compare_vcf" derives the rules from the reference's four loops.
//
// A record is (contig id, 1-based pos, len(REF), len(first ALT), number of ALTs, allele id, genotype pair, QUAL, flags).  Its key is
// (contig id, pos); the keys of a side are distinct, as a dict's are.  Equal allele ids mean equal (REF, first ALT) strings.
// snv = len(REF) == 1 and len(ALT) == 1, ins = len(REF) < len(ALT), del = len(REF) > len(ALT); an MNP is none of the three.
//
//  1. Membership.  A BED set holds a key when one of the contig's merged, sorted [start, end) intervals has start <= pos - 1 < end: the
//     last interval with start <= pos - 1 is the only candidate.  A contig the set has no interval for holds nothing.
//  2. in_fp(key): there is no set, or set 0 (the FP BED) named no contig at all, or set 0 holds the key.
//     in_strat(key): every set from 1 on holds the key (true when there is none; a set that named no contig holds nothing).
//  3. Join.  t(i) is the truth record with the key of input record i, found by binary search in the sorted truth keys; c(j) is the
//     input record with the key of truth record j.  Neither depends on any deletion.
//  4. low_qual(key): high_confident_only, and the key's truth record lacks CTO_CMP_HIGHCONF.  A key without a truth record is never
//     low_qual.  low_af(key): CTO_CMP_LOWAF on either record of the key, or validate_phase 1 and the input record lacks CTO_CMP_H, or
//     validate_phase 2 and it has it.
//  5. Input loop.  Record i is left in the dict (CTO_CMP_KEPT) when in_fp and in_strat and not (benchmark_indel and not low_qual and
//     (snv or number of ALTs > 1)).  input_out_of_bed counts not in_fp; input_out_of_strat counts in_fp and not in_strat.
//  6. Truth loop.  Record j is left when in_fp and (low_qual or (in_strat and not low_af)).  truth_out_of_bed counts not in_fp;
//     truth_out_of_strat counts in_fp, not low_qual and not in_strat.
//  7. A left record is active when its key is neither low_qual nor low_af.  Only active records are classified.
//  8. Active input record i without a left truth record: FP_{snv,ins,del} by its type; in fp_set when snv, or when benchmark_indel and
//     (ins or del).
//  9. Active input record i with a left truth record j: in truth_set.  genotype_match = skip_genotyping or the pairs are equal; a
//     mismatch counts in gt_mismatch.  Equal allele ids and genotype_match: TP_* by i's type; in tp_set when benchmark_indel and
//     (ins or del), or when an SNV true positive exists at or before i in dict order (rule 10).  Otherwise: FP_* by i's type, FN_* by
//     j's type, in fp_set and fn_set; in fp_fn_set when i is snv or j is snv, or benchmark_indel and j is ins or del.
// 10. The running count.  The reference tests `tp_snv or is_snv_truth` with tp_snv the count so far, this record included: the inclusive
//     prefix "any SNV true positive" over dict order.  One exclusive prefix sum of the 0/1 SNV-TP flags (scan.h) plus the record's own.
// 11. Active truth record j whose key no active input record has: FN_* by its type; in fn_set (CTO_CMP_FN of truth_sets) when snv, or
//     benchmark_indel and (ins or del).  The reference's genotype tests against the tuple (0, 0) compare a list and never hold.
// 12. Sweep.  For a cut-off c: the number of fp_set records and of tp_set records with QUAL >= c as doubles.  A NaN on either side
//     never counts.  Device: all pairs, a workgroup keeps 512 cut-offs in registers and streams the QUALs through LDS, partial counts
//     added with integer atomics.  Host: both QUAL lists sorted once, a binary search per cut-off.  The counts are the same integers.
#include <algorithm>
#include <cmath>
#include <mutex>
#include <thread>
#include <vector>
#include "hip_buffers.h"
#include "scan.h"

namespace {

using namespace cto;

enum { C_TP_SNV, C_TP_INS, C_TP_DEL, C_FP_SNV, C_FP_INS, C_FP_DEL, C_FN_SNV, C_FN_INS, C_FN_DEL, C_GT_MISMATCH, C_IN_OOB, C_TR_OOB, C_IN_OOS, C_TR_OOS,
       C_N_IN, C_N_TR };
static_assert(C_N_TR + 1 == CTO_CMP_COUNTERS, "the counters of clairsto_amd.h");
constexpr uint8_t CMP_PENDING = 64;          // tp_set by rule 10 alone: resolved once the prefix is known, never returned
constexpr int CMP_THREADS = 256;
constexpr int SW_THREADS = 256, SW_PER_THREAD = 2, SW_CUTS = SW_THREADS * SW_PER_THREAD, SW_TILE = 1024, SW_CHUNK = 8 * SW_TILE;

struct RecView { const int32_t *ctg, *pos, *ref_len, *alt_len, *n_alt, *allele, *gt; const double* qual; const uint8_t* flags; int64_t n; };
// everything the rules read, on the host or on the device
struct CmpView {
    RecView in, tr;
    const int64_t* tkeys;
    const int32_t* torder;
    int32_t n_sets, n_ctg;
    const int32_t* named;
    const int64_t *off, *start, *end;
    int bi, hc, skip_gt, vp;
    uint32_t *in_member, *tr_member;         // rule 1, one bit per set
    int32_t *t_of, *c_of;                    // rule 3
    int* snv_tp;                             // rule 10's flags
};

__host__ __device__ inline int64_t cmp_key(int32_t ctg, int32_t pos) { return int64_t(uint64_t(uint32_t(ctg)) << 32 | uint32_t(pos)); }

__host__ __device__ inline uint32_t member_bits(const CmpView& V, int32_t ctg, int32_t pos) {
    uint32_t bits = 0;
    if (ctg < 0 || ctg >= V.n_ctg) return 0;
    const int64_t q = int64_t(pos) - 1;
    for (int32_t s = 0; s < V.n_sets; ++s) {
        const int64_t first = V.off[int64_t(s) * V.n_ctg + ctg];
        int64_t lo = first, hi = V.off[int64_t(s) * V.n_ctg + ctg + 1];
        while (lo < hi) {                                            // lo -> one past the last interval with start <= q
            const int64_t mid = lo + (hi - lo) / 2;
            if (V.start[mid] <= q) lo = mid + 1; else hi = mid;
        }
        if (lo > first && V.end[lo - 1] > q) bits |= 1u << s;
    }
    return bits;
}

__host__ __device__ inline int32_t find_truth(const CmpView& V, int64_t key) {
    int64_t lo = 0, hi = V.tr.n;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (V.tkeys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo < V.tr.n && V.tkeys[lo] == key ? V.torder[lo] : -1;
}

__host__ __device__ inline bool in_fp(const CmpView& V, uint32_t bits) { return V.n_sets == 0 || V.named[0] == 0 || (bits & 1u); }
__host__ __device__ inline bool in_strat(const CmpView& V, uint32_t bits) {
    const uint32_t want = V.n_sets > 1 ? ((1u << V.n_sets) - 1u) & ~1u : 0u;
    return (bits & want) == want;
}
__host__ __device__ inline bool low_qual(const CmpView& V, int32_t j) { return V.hc && j >= 0 && !(V.tr.flags[j] & CTO_CMP_HIGHCONF); }
__host__ __device__ inline bool low_af(const CmpView& V, int32_t i, int32_t j) {
    if (j >= 0 && (V.tr.flags[j] & CTO_CMP_LOWAF)) return true;
    if (i < 0) return false;
    const uint8_t f = V.in.flags[i];
    return (f & CTO_CMP_LOWAF) || (V.vp == 1 && !(f & CTO_CMP_H)) || (V.vp == 2 && (f & CTO_CMP_H));
}
__host__ __device__ inline bool input_left(const CmpView& V, int32_t i, bool lowq) {                        // rule 5
    const uint32_t bits = V.in_member[i];
    const bool snv = V.in.ref_len[i] == 1 && V.in.alt_len[i] == 1;
    return in_fp(V, bits) && in_strat(V, bits) && !(V.bi && !lowq && (snv || V.in.n_alt[i] > 1));
}
__host__ __device__ inline bool truth_left(const CmpView& V, int32_t j, bool lowq, bool lowaf) {            // rule 6
    const uint32_t bits = V.tr_member[j];
    return in_fp(V, bits) && (lowq || (in_strat(V, bits) && !lowaf));
}

// rules 1 and 3 for record r of the input (r < in.n) or of the truth
__host__ __device__ inline void cmp_locate(const CmpView& V, int64_t r) {
    if (r < V.in.n) {
        V.in_member[r] = member_bits(V, V.in.ctg[r], V.in.pos[r]);
        V.t_of[r] = find_truth(V, cmp_key(V.in.ctg[r], V.in.pos[r]));
    } else {
        const int64_t j = r - V.in.n;
        V.tr_member[j] = member_bits(V, V.tr.ctg[j], V.tr.pos[j]);
    }
}

// rules 4 to 9 for input record i: its set bits, its counter bits (bit k: one more in counter k)
__host__ __device__ inline uint8_t cmp_input(const CmpView& V, int32_t i, uint32_t* counts) {
    const int32_t j = V.t_of[i];
    const uint32_t bits = V.in_member[i];
    const bool lowq = low_qual(V, j), lowaf = low_af(V, i, j);
    uint32_t cb = 0;
    uint8_t sets = 0;
    V.snv_tp[i] = 0;
    if (!in_fp(V, bits)) cb |= 1u << C_IN_OOB;
    else if (!in_strat(V, bits)) cb |= 1u << C_IN_OOS;
    if (input_left(V, i, lowq)) {
        sets |= CTO_CMP_KEPT;
        cb |= 1u << C_N_IN;
        if (!lowq && !lowaf) {
            const int32_t rl = V.in.ref_len[i], al = V.in.alt_len[i];
            const bool snv = rl == 1 && al == 1, ins = rl < al, del = rl > al, indel = V.bi && (ins || del);
            const uint32_t by_type = snv ? 1u : ins ? 2u : del ? 4u : 0u;
            if (j < 0 || !truth_left(V, j, lowq, lowaf)) {
                cb |= by_type << C_FP_SNV;
                if (snv || indel) sets |= CTO_CMP_FP;
            } else {
                const int32_t trl = V.tr.ref_len[j], tal = V.tr.alt_len[j];
                const bool snv_t = trl == 1 && tal == 1, ins_t = trl < tal, del_t = trl > tal;
                const bool gt_match = V.skip_gt || (V.in.gt[2 * i] == V.tr.gt[2 * j] && V.in.gt[2 * i + 1] == V.tr.gt[2 * j + 1]);
                if (!gt_match) cb |= 1u << C_GT_MISMATCH;
                if (V.in.allele[i] == V.tr.allele[j] && gt_match) {
                    cb |= by_type << C_TP_SNV;
                    if (snv) V.snv_tp[i] = 1;
                    sets |= indel ? CTO_CMP_TP : CMP_PENDING;
                } else {
                    cb |= by_type << C_FP_SNV;
                    cb |= (snv_t ? 1u : ins_t ? 2u : del_t ? 4u : 0u) << C_FN_SNV;
                    sets |= CTO_CMP_FP | CTO_CMP_FN;
                    if (snv || snv_t || (V.bi && (ins_t || del_t))) sets |= CTO_CMP_FP_FN;
                }
                sets |= CTO_CMP_TRUTH;
            }
        }
    }
    *counts = cb;
    return sets;
}

// rules 4, 6, 7 and 11 for truth record j
__host__ __device__ inline uint8_t cmp_truth(const CmpView& V, int32_t j, uint32_t* counts) {
    const int32_t i = V.c_of[j];
    const uint32_t bits = V.tr_member[j];
    const bool lowq = low_qual(V, j), lowaf = low_af(V, i, j);
    uint32_t cb = 0;
    uint8_t sets = 0;
    if (!in_fp(V, bits)) cb |= 1u << C_TR_OOB;
    else if (!lowq && !in_strat(V, bits)) cb |= 1u << C_TR_OOS;
    if (truth_left(V, j, lowq, lowaf)) {
        sets |= CTO_CMP_KEPT;
        cb |= 1u << C_N_TR;
        if (!lowq && !lowaf && !(i >= 0 && input_left(V, i, lowq))) {
            const int32_t trl = V.tr.ref_len[j], tal = V.tr.alt_len[j];
            const bool snv_t = trl == 1 && tal == 1, ins_t = trl < tal, del_t = trl > tal;
            cb |= (snv_t ? 1u : ins_t ? 2u : del_t ? 4u : 0u) << C_FN_SNV;
            if (snv_t || (V.bi && (ins_t || del_t))) sets |= CTO_CMP_FN;
        }
    }
    *counts = cb;
    return sets;
}

// rule 10, once the SNV true positives before record i are counted
__host__ __device__ inline uint8_t cmp_resolve(uint8_t sets, long long before, int own) {
    if (!(sets & CMP_PENDING)) return sets;
    sets &= uint8_t(~CMP_PENDING);
    return before + own > 0 ? uint8_t(sets | CTO_CMP_TP) : sets;
}

// ------------------------------------------------------------------------------------------------ kernels
// One thread per record, the input records first.  c_of takes the largest input index with the key (the keys of a side are distinct,
// so there is one): an integer atomic, the same whatever the order.  c_of is -1 everywhere before the launch.
__global__ __launch_bounds__(CMP_THREADS) void k_cmp_locate(CmpView V) {
    const int64_t r = int64_t(blockIdx.x) * CMP_THREADS + threadIdx.x;
    if (r >= V.in.n + V.tr.n) return;
    cmp_locate(V, r);
    if (r < V.in.n && V.t_of[r] >= 0) atomicMax(&V.c_of[V.t_of[r]], int32_t(r));
}

// One thread per record again.  A wave adds its 16 counters with one ballot each: integer sums, the same whatever the order.
__global__ __launch_bounds__(CMP_THREADS) void k_cmp_classify(CmpView V, uint8_t* __restrict__ in_sets, uint8_t* __restrict__ tr_sets,
                                                              unsigned long long* __restrict__ counters) {
    const int64_t r = int64_t(blockIdx.x) * CMP_THREADS + threadIdx.x;
    uint32_t cb = 0;
    if (r < V.in.n) in_sets[r] = cmp_input(V, int32_t(r), &cb);
    else if (r < V.in.n + V.tr.n) tr_sets[r - V.in.n] = cmp_truth(V, int32_t(r - V.in.n), &cb);
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < CTO_CMP_COUNTERS; ++k) {
        const unsigned long long m = __ballot((cb >> k) & 1u);
        if (lane == 0 && m) atomicAdd(&counters[k], (unsigned long long)__popcll(m));
    }
}

__global__ __launch_bounds__(CMP_THREADS) void k_cmp_resolve(uint8_t* __restrict__ in_sets, const long long* __restrict__ before,
                                                             const int* __restrict__ snv_tp, int64_t n) {
    const int64_t i = int64_t(blockIdx.x) * CMP_THREADS + threadIdx.x;
    if (i < n) in_sets[i] = cmp_resolve(in_sets[i], before[i], snv_tp[i]);
}

// Rule 12.  blockIdx.x picks SW_CUTS cut-offs, two per thread in registers (a cut-off past the end is a NaN: nothing counts against it);
// blockIdx.y picks SW_CHUNK values, which go through LDS SW_TILE at a time as two arrays: the QUAL where the record is in fp_set (tp_set),
// a NaN where it is not.  Every lane reads the same LDS word at the same time (a broadcast, no bank conflict).  16 KiB of LDS.
__global__ __launch_bounds__(SW_THREADS) void k_cmp_sweep(const double* __restrict__ qual, const uint8_t* __restrict__ sets, int64_t n,
                                                          const double* __restrict__ cut, int64_t n_cut, unsigned long long* __restrict__ out) {
    __shared__ double v_fp[SW_TILE], v_tp[SW_TILE];
    const int t = threadIdx.x;
    int64_t k[SW_PER_THREAD];
    double c[SW_PER_THREAD];
    unsigned f[SW_PER_THREAD], p[SW_PER_THREAD];
#pragma unroll
    for (int u = 0; u < SW_PER_THREAD; ++u) {
        k[u] = int64_t(blockIdx.x) * SW_CUTS + u * SW_THREADS + t;
        c[u] = k[u] < n_cut ? cut[k[u]] : NAN;
        f[u] = p[u] = 0;
    }
    const int64_t lo = int64_t(blockIdx.y) * SW_CHUNK, hi = lo + SW_CHUNK < n ? lo + SW_CHUNK : n;
    for (int64_t base = lo; base < hi; base += SW_TILE) {
        const int len = int(hi - base < SW_TILE ? hi - base : SW_TILE);
        __syncthreads();                                             // the tile before is read to its end
        for (int e = t; e < len; e += SW_THREADS) {
            const double v = qual[base + e];
            const uint8_t s = sets[base + e];
            v_fp[e] = (s & CTO_CMP_FP) ? v : NAN;
            v_tp[e] = (s & CTO_CMP_TP) ? v : NAN;
        }
        __syncthreads();
        for (int e = 0; e < len; ++e) {
            const double a = v_fp[e], b = v_tp[e];
#pragma unroll
            for (int u = 0; u < SW_PER_THREAD; ++u) {
                f[u] += a >= c[u];
                p[u] += b >= c[u];
            }
        }
    }
#pragma unroll
    for (int u = 0; u < SW_PER_THREAD; ++u)
        if (k[u] < n_cut) {
            if (f[u]) atomicAdd(&out[2 * k[u]], (unsigned long long)f[u]);
            if (p[u]) atomicAdd(&out[2 * k[u] + 1], (unsigned long long)p[u]);
        }
}

void launch_sweep(hipStream_t s, const double* qual, const uint8_t* sets, int64_t n, const double* cut, int64_t n_cut, int64_t* out) {
    if (n == 0 || n_cut == 0) return;                                // the counts were zeroed
    const dim3 grid(uint32_t(cdiv(n_cut, SW_CUTS)), uint32_t(cdiv(n, SW_CHUNK)));
    hipLaunchKernelGGL(k_cmp_sweep, grid, dim3(SW_THREADS), 0, s, qual, sets, n, cut, n_cut, reinterpret_cast<unsigned long long*>(out));
}

// ------------------------------------------------------------------------------------------------ host path
template <class F> void over_threads(int64_t n_items, int host_threads, F&& range) {      // range(t, lo, hi) over contiguous parts
    const unsigned hw = std::thread::hardware_concurrency();
    const int64_t cap = host_threads > 0 ? host_threads : std::min<int64_t>(hw ? hw : 1, 16);
    const int64_t n_threads = std::max<int64_t>(1, std::min<int64_t>(cap, cdiv(n_items, 4096)));
    const int64_t per = cdiv(n_items, n_threads);
    std::vector<std::thread> threads;
    for (int64_t t = 1; t < n_threads; ++t) threads.emplace_back(range, int(t), std::min(n_items, t * per), std::min(n_items, (t + 1) * per));
    range(0, int64_t(0), std::min(n_items, per));
    for (auto& th : threads) th.join();
}

void host_sweep(const double* qual, const uint8_t* sets, int64_t n, const double* cut, int64_t n_cut, int host_threads, int64_t* out) {
    std::vector<double> v[2];
    for (int64_t i = 0; i < n; ++i) {
        if (qual[i] != qual[i]) continue;
        if (sets[i] & CTO_CMP_FP) v[0].push_back(qual[i]);
        if (sets[i] & CTO_CMP_TP) v[1].push_back(qual[i]);
    }
    std::sort(v[0].begin(), v[0].end());
    std::sort(v[1].begin(), v[1].end());
    over_threads(n_cut, host_threads, [&](int, int64_t lo, int64_t hi) {
        for (int64_t k = lo; k < hi; ++k)
            for (int w = 0; w < 2; ++w)
                out[2 * k + w] = cut[k] != cut[k] ? 0 : int64_t(v[w].end() - std::lower_bound(v[w].begin(), v[w].end(), cut[k]));
    });
}

void host_compare(CmpView V, int host_threads, uint8_t* in_sets, uint8_t* tr_sets, int64_t* counters) {
    const int64_t n_in = V.in.n, n_tr = V.tr.n;
    over_threads(n_in + n_tr, host_threads, [&](int, int64_t lo, int64_t hi) { for (int64_t r = lo; r < hi; ++r) cmp_locate(V, r); });
    std::fill(V.c_of, V.c_of + n_tr, -1);
    for (int64_t i = 0; i < n_in; ++i)
        if (V.t_of[i] >= 0) V.c_of[V.t_of[i]] = std::max(V.c_of[V.t_of[i]], int32_t(i));
    std::mutex mu;
    over_threads(n_in + n_tr, host_threads, [&](int, int64_t lo, int64_t hi) {
        int64_t local[CTO_CMP_COUNTERS] = {0};
        for (int64_t r = lo; r < hi; ++r) {
            uint32_t cb = 0;
            if (r < n_in) in_sets[r] = cmp_input(V, int32_t(r), &cb);
            else tr_sets[r - n_in] = cmp_truth(V, int32_t(r - n_in), &cb);
            for (int k = 0; k < CTO_CMP_COUNTERS; ++k) local[k] += (cb >> k) & 1u;
        }
        std::lock_guard<std::mutex> lock(mu);
        for (int k = 0; k < CTO_CMP_COUNTERS; ++k) counters[k] += local[k];
    });
    long long before = 0;
    for (int64_t i = 0; i < n_in; ++i) {
        in_sets[i] = cmp_resolve(in_sets[i], before, V.snv_tp[i]);
        before += V.snv_tp[i];
    }
}

// ------------------------------------------------------------------------------------------------ entry points
int check_records(const char* who, const cto_compare_records* R, bool need_qual, int32_t n_sets, int32_t n_ctg) {
    CTO_REQUIRE(R && R->n >= 0 && R->n <= CTO_CMP_MAX_RECORDS, CTO_EINVAL, "cto_compare_calls: %s: bad record count", who);
    CTO_REQUIRE(R->n == 0 || (R->ctg && R->pos && R->ref_len && R->alt_len && R->n_alt && R->allele && R->gt && R->flags && (R->qual || !need_qual)),
                CTO_EINVAL, "cto_compare_calls: %s: null array", who);
    for (int64_t i = 0; i < R->n; ++i)
        CTO_REQUIRE(R->ctg[i] >= 0 && (n_sets == 0 || R->ctg[i] < n_ctg), CTO_EINVAL, "cto_compare_calls: %s record %lld: contig id %d", who,
                    (long long)i, R->ctg[i]);
    return CTO_OK;
}

int check_beds(const cto_compare_beds* B, int64_t* n_iv) {
    *n_iv = 0;
    CTO_REQUIRE(B && B->n_sets >= 0 && B->n_sets <= CTO_CMP_MAX_SETS && B->n_ctg >= 0, CTO_EINVAL, "cto_compare_calls: BED sets: bad counts");
    if (B->n_sets == 0) return CTO_OK;
    CTO_REQUIRE(B->named && B->off, CTO_EINVAL, "cto_compare_calls: BED sets: null array");
    const int64_t n_off = int64_t(B->n_sets) * B->n_ctg;
    CTO_REQUIRE(B->off[0] == 0, CTO_EINVAL, "cto_compare_calls: BED sets: offsets start at 0");
    for (int64_t k = 0; k < n_off; ++k) CTO_REQUIRE(B->off[k] <= B->off[k + 1], CTO_EINVAL, "cto_compare_calls: BED sets: offsets must ascend");
    *n_iv = B->off[n_off];
    CTO_REQUIRE(*n_iv <= CTO_CMP_MAX_RECORDS && (*n_iv == 0 || (B->start && B->end)), CTO_EINVAL, "cto_compare_calls: BED sets: bad intervals");
    for (int64_t k = 0; k < n_off; ++k)
        for (int64_t a = B->off[k]; a < B->off[k + 1]; ++a)
            CTO_REQUIRE(B->start[a] < B->end[a] && (a == B->off[k] || B->end[a - 1] <= B->start[a]), CTO_EINVAL,
                        "cto_compare_calls: BED sets: interval %lld is empty, unsorted or overlaps the one before", (long long)a);
    return CTO_OK;
}

struct CmpContext : BatchCtx { DevBuf d_tmp; };

// lays arrays out behind each other in the upload block, 16-byte aligned
struct Block {
    struct Part { const void* src; size_t bytes, at; };
    std::vector<Part> parts;
    size_t bytes = 0;
    size_t add(const void* src, size_t n) { const size_t at = bytes; parts.push_back({src, n, at}); bytes = align16(bytes + n); return at; }
    void fill(char* h) const { for (const Part& p : parts) if (p.bytes && p.src) memcpy(h + p.at, p.src, p.bytes); }
};

struct RecAt { size_t ctg, pos, ref_len, alt_len, n_alt, allele, gt, qual, flags; };
RecAt add_records(Block& b, const cto_compare_records* R) {
    const size_t n = size_t(R->n);
    RecAt a;
    a.ctg = b.add(R->ctg, n * 4); a.pos = b.add(R->pos, n * 4); a.ref_len = b.add(R->ref_len, n * 4); a.alt_len = b.add(R->alt_len, n * 4);
    a.n_alt = b.add(R->n_alt, n * 4); a.allele = b.add(R->allele, n * 4); a.gt = b.add(R->gt, n * 8); a.qual = b.add(R->qual, R->qual ? n * 8 : 0);
    a.flags = b.add(R->flags, n);
    return a;
}
RecView view_records(const char* base, const RecAt& a, int64_t n) {
    auto i32 = [&](size_t at) { return reinterpret_cast<const int32_t*>(base + at); };
    return RecView{i32(a.ctg), i32(a.pos), i32(a.ref_len), i32(a.alt_len), i32(a.n_alt), i32(a.allele), i32(a.gt),
                   reinterpret_cast<const double*>(base + a.qual), reinterpret_cast<const uint8_t*>(base + a.flags), n};
}

}  // namespace

extern "C" int cto_compare_calls(const cto_compare_records* input, const cto_compare_records* truth, const int64_t* truth_sorted_keys,
                                 const int32_t* truth_order, const cto_compare_beds* beds, int benchmark_indel, int high_confident_only,
                                 int skip_genotyping, int validate_phase, const double* cutoffs, int64_t n_cutoffs, const double* roc_cutoffs,
                                 int64_t n_roc, int where, int host_threads, void* stream, uint8_t* input_sets, uint8_t* truth_sets,
                                 int64_t* counters, int64_t* sweep, int64_t* roc_sweep, cto_compare_stats* stats) try {
    if (stats) *stats = cto_compare_stats{0, 0, 0, 0, 0.0};
    CTO_REQUIRE(where == 0 || where == 1, CTO_EINVAL, "cto_compare_calls: where is %d, not 0 (device) or 1 (host)", where);
    CTO_REQUIRE(validate_phase >= 0 && validate_phase <= 2, CTO_EINVAL, "cto_compare_calls: validate_phase is %d, not 0, 1 or 2", validate_phase);
    int64_t n_iv = 0;
    if (const int rc = check_beds(beds, &n_iv)) return rc;
    if (const int rc = check_records("input", input, n_cutoffs + n_roc > 0, beds->n_sets, beds->n_ctg)) return rc;
    if (const int rc = check_records("truth", truth, false, beds->n_sets, beds->n_ctg)) return rc;
    const int64_t n_in = input->n, n_tr = truth->n;
    CTO_REQUIRE(n_cutoffs >= 0 && n_roc >= 0 && n_cutoffs <= CTO_CMP_MAX_CUTOFFS && n_roc <= CTO_CMP_MAX_CUTOFFS, CTO_EINVAL,
                "cto_compare_calls: %lld and %lld cut-offs", (long long)n_cutoffs, (long long)n_roc);
    CTO_REQUIRE(counters && (n_in == 0 || input_sets) && (n_tr == 0 || (truth_sets && truth_sorted_keys && truth_order)) &&
                (n_cutoffs == 0 || (cutoffs && sweep)) && (n_roc == 0 || (roc_cutoffs && roc_sweep)), CTO_EINVAL, "cto_compare_calls: null array");
    for (int64_t k = 0; k < n_tr; ++k) {                             // what the join and the scatter into c_of rely on
        const int32_t j = truth_order[k];
        CTO_REQUIRE(j >= 0 && j < n_tr && truth_sorted_keys[k] == cmp_key(truth->ctg[j], truth->pos[j]) &&
                    (k == 0 || truth_sorted_keys[k - 1] < truth_sorted_keys[k]), CTO_EINVAL,
                    "cto_compare_calls: the sorted truth keys must ascend strictly and name their records (entry %lld)", (long long)k);
    }
    if (stats) { stats->n_input = n_in; stats->n_truth = n_tr; stats->n_cutoffs = n_cutoffs + n_roc; stats->host_path = where; }
    std::fill(counters, counters + CTO_CMP_COUNTERS, int64_t(0));
    if (n_cutoffs) std::fill(sweep, sweep + 2 * n_cutoffs, int64_t(0));
    if (n_roc) std::fill(roc_sweep, roc_sweep + 2 * n_roc, int64_t(0));

    CmpView V{};
    V.n_sets = beds->n_sets; V.n_ctg = beds->n_ctg;
    V.bi = benchmark_indel != 0; V.hc = high_confident_only != 0; V.skip_gt = skip_genotyping != 0; V.vp = validate_phase;
    if (where == 1) {
        V.in = RecView{input->ctg, input->pos, input->ref_len, input->alt_len, input->n_alt, input->allele, input->gt, input->qual, input->flags, n_in};
        V.tr = RecView{truth->ctg, truth->pos, truth->ref_len, truth->alt_len, truth->n_alt, truth->allele, truth->gt, truth->qual, truth->flags, n_tr};
        V.tkeys = truth_sorted_keys; V.torder = truth_order;
        V.named = beds->named; V.off = beds->off; V.start = beds->start; V.end = beds->end;
        std::vector<uint32_t> in_member(size_t(n_in) + 1), tr_member(size_t(n_tr) + 1);
        std::vector<int32_t> t_of(size_t(n_in) + 1), c_of(size_t(n_tr) + 1);
        std::vector<int> snv_tp(size_t(n_in) + 1);
        V.in_member = in_member.data(); V.tr_member = tr_member.data(); V.t_of = t_of.data(); V.c_of = c_of.data(); V.snv_tp = snv_tp.data();
        host_compare(V, host_threads, input_sets, truth_sets, counters);
        if (n_cutoffs) host_sweep(input->qual, input_sets, n_in, cutoffs, n_cutoffs, host_threads, sweep);
        if (n_roc) host_sweep(input->qual, input_sets, n_in, roc_cutoffs, n_roc, host_threads, roc_sweep);
        return CTO_OK;
    }

    int n_dev = 0;
    CTO_REQUIRE(hipGetDeviceCount(&n_dev) == hipSuccess && n_dev > 0, CTO_EHIP,
                "cto_compare_calls: no HIP device (the host path is taken only when asked for)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    // one upload: both record tables, the sorted keys, the BED sets, the cut-offs; one download: [counters | sweep | roc | input sets | truth sets]
    Block up;
    const RecAt at_in = add_records(up, input), at_tr = add_records(up, truth);
    const size_t at_keys = up.add(truth_sorted_keys, size_t(n_tr) * 8), at_order = up.add(truth_order, size_t(n_tr) * 4);
    const size_t n_off = beds->n_sets ? size_t(beds->n_sets) * beds->n_ctg + 1 : 0;
    const size_t at_named = up.add(beds->named, size_t(beds->n_sets) * 4), at_off = up.add(beds->off, n_off * 8);
    const size_t at_start = up.add(beds->start, size_t(n_iv) * 8), at_end = up.add(beds->end, size_t(n_iv) * 8);
    const size_t at_cut = up.add(cutoffs, size_t(n_cutoffs) * 8), at_roc = up.add(roc_cutoffs, size_t(n_roc) * 8);
    const size_t o_sweep = size_t(CTO_CMP_COUNTERS) * 8, o_roc = o_sweep + size_t(n_cutoffs) * 16, o_in = o_roc + size_t(n_roc) * 16,
                 o_tr = align16(o_in + size_t(n_in)), bytes_out = align16(o_tr + size_t(n_tr));
    // scratch: [before (n_in + 1) x 8 | tile sums | tile total | in_member | tr_member | t_of | c_of | snv_tp]
    const size_t tiles = size_t(cdiv(n_in, SCAN_TILE)) + 1;
    const size_t t_tiles = align16((size_t(n_in) + 1) * 8), t_total = t_tiles + align16(tiles * 8), t_inm = t_total + 16,
                 t_trm = t_inm + align16(size_t(n_in) * 4), t_tof = t_trm + align16(size_t(n_tr) * 4), t_cof = t_tof + align16(size_t(n_in) * 4),
                 t_snv = t_cof + align16(size_t(n_tr) * 4), bytes_tmp = t_snv + align16(size_t(n_in) * 4);
    CmpContext& X = process_wide<CmpContext>();
    std::lock_guard<std::mutex> lock(X.mu);
    if (const int rc = X.open(up.bytes + 16, bytes_out)) return rc;
    if (const int rc = X.d_tmp.ensure(bytes_tmp)) return rc;
    up.fill(X.h_in.as<char>());
    const char* din = X.d_in.as<char>();
    char *dout = X.d_out.as<char>(), *tmp = X.d_tmp.as<char>();
    V.in = view_records(din, at_in, n_in);
    V.tr = view_records(din, at_tr, n_tr);
    V.tkeys = reinterpret_cast<const int64_t*>(din + at_keys); V.torder = reinterpret_cast<const int32_t*>(din + at_order);
    V.named = reinterpret_cast<const int32_t*>(din + at_named); V.off = reinterpret_cast<const int64_t*>(din + at_off);
    V.start = reinterpret_cast<const int64_t*>(din + at_start); V.end = reinterpret_cast<const int64_t*>(din + at_end);
    V.in_member = reinterpret_cast<uint32_t*>(tmp + t_inm); V.tr_member = reinterpret_cast<uint32_t*>(tmp + t_trm);
    V.t_of = reinterpret_cast<int32_t*>(tmp + t_tof); V.c_of = reinterpret_cast<int32_t*>(tmp + t_cof); V.snv_tp = reinterpret_cast<int*>(tmp + t_snv);
    long long* before = reinterpret_cast<long long*>(tmp);
    uint8_t *d_in_sets = reinterpret_cast<uint8_t*>(dout + o_in), *d_tr_sets = reinterpret_cast<uint8_t*>(dout + o_tr);

    if (up.bytes) CTO_HIP(hipMemcpyAsync(X.d_in.p, X.h_in.p, up.bytes, hipMemcpyHostToDevice, s));
    CTO_HIP(hipEventRecord(X.ev0, s));
    CTO_HIP(hipMemsetAsync(dout, 0, bytes_out, s));
    if (n_tr) CTO_HIP(hipMemsetAsync(V.c_of, 0xff, size_t(n_tr) * 4, s));
    if (n_in + n_tr) {
        const dim3 grid(uint32_t(cdiv(n_in + n_tr, CMP_THREADS))), block(CMP_THREADS);
        hipLaunchKernelGGL(k_cmp_locate, grid, block, 0, s, V);
        hipLaunchKernelGGL(k_cmp_classify, grid, block, 0, s, V, d_in_sets, d_tr_sets, reinterpret_cast<unsigned long long*>(dout));
    }
    if (n_in) {
        scan_exclusive<long long>(s, V.snv_tp, int(n_in), before, static_cast<long long*>(nullptr), reinterpret_cast<long long*>(tmp + t_tiles),
                                  reinterpret_cast<long long*>(tmp + t_total));
        hipLaunchKernelGGL(k_cmp_resolve, dim3(uint32_t(cdiv(n_in, CMP_THREADS))), dim3(CMP_THREADS), 0, s, d_in_sets, before, V.snv_tp, n_in);
    }
    launch_sweep(s, V.in.qual, d_in_sets, n_in, reinterpret_cast<const double*>(din + at_cut), n_cutoffs, reinterpret_cast<int64_t*>(dout + o_sweep));
    launch_sweep(s, V.in.qual, d_in_sets, n_in, reinterpret_cast<const double*>(din + at_roc), n_roc, reinterpret_cast<int64_t*>(dout + o_roc));
    CTO_HIP(hipGetLastError());
    CTO_HIP(hipEventRecord(X.ev1, s));
    CTO_HIP(hipMemcpyAsync(X.h_out.p, X.d_out.p, bytes_out, hipMemcpyDeviceToHost, s));
    CTO_HIP(record_and_wait(X.done, s));
    if (stats) {
        float ms = 0.f;
        CTO_HIP(hipEventElapsedTime(&ms, X.ev0, X.ev1));
        stats->kernel_ms = ms;
    }
    const char* ho = X.h_out.as<char>();
    memcpy(counters, ho, size_t(CTO_CMP_COUNTERS) * 8);
    if (n_cutoffs) memcpy(sweep, ho + o_sweep, size_t(n_cutoffs) * 16);
    if (n_roc) memcpy(roc_sweep, ho + o_roc, size_t(n_roc) * 16);
    if (n_in) memcpy(input_sets, ho + o_in, size_t(n_in));
    if (n_tr) memcpy(truth_sets, ho + o_tr, size_t(n_tr));
    return CTO_OK;
}
CTO_CATCH("cto_compare_calls", int)

// rule 12 alone: out[2k], out[2k + 1] = the values with CTO_CMP_FP, with CTO_CMP_TP in `sets` that are >= cutoffs[k]; for the tests
extern "C" int cto_compare_sweep(const double* values, const uint8_t* sets, int64_t n, const double* cutoffs, int64_t n_cutoffs, int where,
                                 int host_threads, void* stream, int64_t* out) try {
    CTO_REQUIRE(where == 0 || where == 1, CTO_EINVAL, "cto_compare_sweep: where is %d, not 0 (device) or 1 (host)", where);
    CTO_REQUIRE(n >= 0 && n <= CTO_CMP_MAX_RECORDS && n_cutoffs >= 0 && n_cutoffs <= CTO_CMP_MAX_CUTOFFS && (n == 0 || (values && sets)) &&
                (n_cutoffs == 0 || (cutoffs && out)), CTO_EINVAL, "cto_compare_sweep: bad arguments");
    if (n_cutoffs == 0) return CTO_OK;
    std::fill(out, out + 2 * n_cutoffs, int64_t(0));
    if (where == 1) {
        host_sweep(values, sets, n, cutoffs, n_cutoffs, host_threads, out);
        return CTO_OK;
    }
    int n_dev = 0;
    CTO_REQUIRE(hipGetDeviceCount(&n_dev) == hipSuccess && n_dev > 0, CTO_EHIP,
                "cto_compare_sweep: no HIP device (the host path is taken only when asked for)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    Block up;
    const size_t at_v = up.add(values, size_t(n) * 8), at_c = up.add(cutoffs, size_t(n_cutoffs) * 8), at_s = up.add(sets, size_t(n));
    const size_t bytes_out = size_t(n_cutoffs) * 16;
    CmpContext& X = process_wide<CmpContext>();
    std::lock_guard<std::mutex> lock(X.mu);
    if (const int rc = X.open(up.bytes + 16, bytes_out)) return rc;
    up.fill(X.h_in.as<char>());
    const char* din = X.d_in.as<char>();
    CTO_HIP(hipMemcpyAsync(X.d_in.p, X.h_in.p, up.bytes, hipMemcpyHostToDevice, s));
    CTO_HIP(hipMemsetAsync(X.d_out.p, 0, bytes_out, s));
    launch_sweep(s, reinterpret_cast<const double*>(din + at_v), reinterpret_cast<const uint8_t*>(din + at_s), n,
                 reinterpret_cast<const double*>(din + at_c), n_cutoffs, X.d_out.as<int64_t>());
    CTO_HIP(hipGetLastError());
    CTO_HIP(hipMemcpyAsync(X.h_out.p, X.d_out.p, bytes_out, hipMemcpyDeviceToHost, s));
    CTO_HIP(record_and_wait(X.done, s));
    memcpy(out, X.h_out.p, bytes_out);
    return CTO_OK;
}
CTO_CATCH("cto_compare_sweep", int)
