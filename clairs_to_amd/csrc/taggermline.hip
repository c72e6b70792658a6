// tag_germline_variant, the last step of the Verdict chain (src/verdict/tag_germline_variant.py:78-111 of the reference): per PASS call
// the first copy-number segment that holds it, the up to four allele fractions that segment and the purity predict, and the exact
// two-sided binomial test of the call's read counts against each - the kernel, the host path of the same call, the entry points.
// Compiled with -ffp-contract=off: every product, quotient and sum below is an fp64 operation of its own, the same bits on the host and
// on gfx950.  Nothing here calls log, exp, lgamma or pow.  DESIGN.md "Germline tagging" derives the three rules.
//
// 1. Segment rule.  The smallest i with seg_chr[i] == ctg and seg_start[i] <= pos <= seg_end[i]: file order, so that tables which
//    overlap or are not sorted give what the reference's linear scan gives.  -1 when there is none: no fraction, no test, NaN everywhere.
// 2. Fraction rule.  p = purity, M = nMinor, C = nMajor + nMinor; M = C - M when M == 0;  den = (p * C + 2 * (1 - p)) + DBL_EPSILON;
//      AF_G1 = (p * M + (1 - p)) / den,  AF_S1 = (p * M + 0.0) / den,
//      AF_G2 = (p * (C - M) + (1 - p)) / den  unless M == C - M (then AF_G2, AF_S2, P_G2, P_S2 are NaN),
//      AF_S2 = (p * (C - M) + 0.0) / den      unless C - M == 0 (then AF_S2, P_S2 are NaN);
//    k = rint(n * AF) (half to even: Python's round) successes in n = depth trials are tested against each.
// 3. Test rule (scipy.stats.binomtest, two-sided, as a ratio of sums).  p == 0: 1 if k == 0 else 0.  p == 1: 1 if k == n else 0.
//    k == p * n in fp64: 1.  Otherwise, with r = p / (1 - p), the anchor a = floor((n + 1) * p) held within [floor(p * n), ceil(p * n)]
//    and at most n, and the weights relative to it
//      w(a) = 1,  w(i + 1) = w(i) * (((n - i) * r) / (i + 1)) going up,  w(i - 1) = w(i) * (i / ((n - i + 1) * r)) going down,
//    the value is min(1, num / den): den sums every weight; num sums, on k's side of p * n, the weights from the end up to k (by index),
//    and on the other side the weights at or beyond ceil(p * n) (k below) or floor(p * n) (k above) with w(i) <= w(k) * (1 + 1e-7).
//    One fixed order: a side is cut into blocks of 64 consecutive ratios; a block's prefix products come from the scan
//    x[j] = x[j - o] * x[j] (j >= o) for o = 1, 2, 4, .. 32, then w = carry * x with the carry the last weight of the block before
//    (1 at first); a block's two sums are the tree ((s0 + s1) + (s2 + s3)) + ... over its 64 places, a place beyond the side or left out
//    counting as 0.0; num and den start from the anchor's term and take the block sums in order, k's side first (the down side when k
//    is the anchor).  A side ends early once a carry is 0.0: everything beyond is 0.0 too.  Weights go through the subnormals to zero
//    far from the anchor; that is right, and the same on both paths.  O(n) per test.
//    Errors, in scipy's words: n < 1, k < 0 or k > n, p outside [0, 1] (a NaN included).
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <mutex>
#include <thread>
#include <vector>
#include "hip_buffers.h"

namespace {

using namespace cto;

constexpr int TG_WAVE = 64, TG_WAVES = CTO_TAG_WAVES_PER_GROUP, TG_THREADS = TG_WAVE * TG_WAVES;
constexpr double TG_RERR = 1 + 1e-7;
enum { TG_FINE = 0, TG_BAD_N = 1, TG_BAD_K = 2, TG_BAD_P = 3 };

// what of a test does not depend on the path
struct BtPlan {
    int status;          // TG_*
    int decided;         // the value is `value` already
    double value;
    int low;             // k < p * n
    int64_t a, edge;     // the anchor; ceil(p * n) when low, else floor(p * n)
    double r;
};

__host__ __device__ inline BtPlan bt_plan(int64_t k, int64_t n, double p) {
    BtPlan pl = {TG_FINE, 1, 0.0, 0, 0, 0, 0.0};
    if (n < 1) { pl.status = TG_BAD_N; return pl; }
    if (k < 0 || k > n) { pl.status = TG_BAD_K; return pl; }
    if (!(p >= 0.0 && p <= 1.0)) { pl.status = TG_BAD_P; return pl; }
    if (p == 0.0) { pl.value = k == 0 ? 1.0 : 0.0; return pl; }
    if (p == 1.0) { pl.value = k == n ? 1.0 : 0.0; return pl; }
    const double pn = p * double(n), kd = double(k);
    if (kd == pn) { pl.value = 1.0; return pl; }
    const int64_t lo = int64_t(floor(pn)), hi = int64_t(ceil(pn));
    int64_t a = int64_t(floor(double(n + 1) * p));
    a = a < lo ? lo : a;
    a = a > hi ? hi : a;
    a = a > n ? n : a;
    pl.decided = 0;
    pl.low = kd < pn;
    pl.a = a;
    pl.edge = pl.low ? hi : lo;
    pl.r = p / (1.0 - p);
    return pl;
}

// the t-th ratio of a side and the index of the weight it leads to
__host__ __device__ inline double bt_ratio(bool up, int64_t a, int64_t n, double r, int64_t t, int64_t* idx) {
    if (up) {
        const int64_t i = a + t;
        *idx = i + 1;
        return (double(n - i) * r) / double(i + 1);
    }
    const int64_t i = a - t;
    *idx = i - 1;
    return double(i) / (double(n - i + 1) * r);
}

// the fractions of a call in segment (nmaj, nmin): af[0..4) = G1, S1, G2, S2
__host__ __device__ inline void tg_fractions(double p, int64_t nmaj, int64_t nmin, double af[4]) {
    int64_t M = nmin;
    const int64_t C = nmaj + nmin;
    if (M == 0) M = C - M;
    const double q = 1.0 - p, den = (p * double(C) + 2.0 * q) + DBL_EPSILON;
    af[0] = (p * double(M) + q) / den;
    af[1] = (p * double(M) + 0.0) / den;
    af[2] = af[3] = NAN;
    if (M != C - M) {
        af[2] = (p * double(C - M) + q) / den;
        if (C - M != 0) af[3] = (p * double(C - M) + 0.0) / den;
    }
}

// rint(n * AF) as an integer; out of int64's reach (a NaN included) becomes -1, which no test accepts
__host__ __device__ inline int64_t tg_successes(int64_t n, double af) {
    const double k = rint(double(n) * af);
    return k >= 0.0 && k <= 4294967296.0 ? int64_t(k) : -1;
}

// ------------------------------------------------------------------------------------------------ host path
struct HostSums { double num, den, wk; };

void host_side(bool up, const BtPlan& pl, int64_t k, int64_t n, bool by_index, double thr, HostSums& s) {
    const int64_t len = up ? n - pl.a : pl.a;
    double carry = 1.0, x[TG_WAVE], sn[TG_WAVE], sd[TG_WAVE];
    int64_t idx[TG_WAVE];
    for (int64_t b0 = 0; b0 < len; b0 += TG_WAVE) {
        for (int j = 0; j < TG_WAVE; ++j) {
            idx[j] = -1;
            x[j] = b0 + j < len ? bt_ratio(up, pl.a, n, pl.r, b0 + j, &idx[j]) : 0.0;
        }
        for (int o = 1; o < TG_WAVE; o <<= 1)
            for (int j = TG_WAVE - 1; j >= o; --j) x[j] = x[j - o] * x[j];
        for (int j = 0; j < TG_WAVE; ++j) {
            const double w = carry * x[j];
            const bool in_side = b0 + j < len;
            if (by_index && in_side && idx[j] == k) s.wk = w;
            const bool inc = in_side && (by_index ? (up ? idx[j] >= k : idx[j] <= k) : w <= thr);
            x[j] = w;
            sd[j] = w;
            sn[j] = inc ? w : 0.0;
        }
        for (int width = TG_WAVE / 2; width >= 1; width >>= 1)
            for (int j = 0; j < width; ++j) {
                sd[j] = sd[2 * j] + sd[2 * j + 1];
                sn[j] = sn[2 * j] + sn[2 * j + 1];
            }
        s.den += sd[0];
        s.num += sn[0];
        carry = x[TG_WAVE - 1];
        if (carry == 0.0) break;
    }
}

double host_binom(const BtPlan& pl, int64_t k, int64_t n) {
    if (pl.decided) return pl.value;
    HostSums s = {0.0, 1.0, k == pl.a ? 1.0 : 0.0};
    const bool near_up = !pl.low;                                // k's side of the anchor
    HostSums first = {0.0, 0.0, s.wk};
    host_side(near_up, pl, k, n, true, 0.0, first);
    const double thr = first.wk * TG_RERR;
    const bool anchor_in = (pl.low ? pl.a <= k : pl.a >= k) || ((pl.low ? pl.a >= pl.edge : pl.a <= pl.edge) && 1.0 <= thr);
    s.num = anchor_in ? 1.0 : 0.0;
    s.num += first.num;
    s.den += first.den;
    HostSums second = {0.0, 0.0, 0.0};
    host_side(!near_up, pl, k, n, false, thr, second);
    s.num += second.num;
    s.den += second.den;
    const double v = s.num / s.den;
    return v < 1.0 ? v : 1.0;
}

template <class F> void over_threads(size_t n_items, F&& item) {          // item(i) for every i, on at most 16 threads
    const unsigned hw = std::thread::hardware_concurrency();
    const size_t n_threads = std::max<size_t>(1, std::min<size_t>({size_t(hw ? hw : 1), size_t(16), n_items}));
    auto work = [&](size_t t) {
        for (size_t i = t; i < n_items; i += n_threads) item(i);
    };
    std::vector<std::thread> threads;
    for (size_t t = 1; t < n_threads; ++t) threads.emplace_back(work, t);
    work(0);
    for (auto& th : threads) th.join();
}

struct SegTable { const int32_t* chr; const int64_t *start, *end, *nmaj, *nmin; int64_t S; };

// one call on the host: seg, status, af[4], pv[4]
void host_call(const SegTable& T, double purity, int32_t ctg, int64_t pos, int64_t n, double freq, int32_t* seg, int32_t* status, double* af, double* pv) {
    *seg = -1;
    *status = TG_FINE;
    for (int j = 0; j < 4; ++j) af[j] = pv[j] = NAN;
    for (int64_t i = 0; i < T.S; ++i)
        if (T.chr[i] == ctg && T.start[i] <= pos && pos <= T.end[i]) {
            *seg = int32_t(i);
            break;
        }
    if (*seg < 0) return;
    tg_fractions(purity, T.nmaj[*seg], T.nmin[*seg], af);
    const int64_t k = tg_successes(n, freq);
    for (int j = 0; j < 4; ++j) {
        if (af[j] != af[j]) continue;
        const BtPlan pl = bt_plan(k, n, af[j]);
        if (pl.status != TG_FINE) {
            if (*status == TG_FINE) *status = pl.status;
            continue;
        }
        pv[j] = host_binom(pl, k, n);
    }
}

// ------------------------------------------------------------------------------------------------ kernel
struct WaveSums { double num, den, wk; };

// one side of a test by the 64 lanes of a wave; every lane ends with the same sums
__device__ inline void wave_side(bool up, const BtPlan& pl, int64_t k, int64_t n, bool by_index, double thr, int lane, WaveSums& s) {
    const int64_t len = up ? n - pl.a : pl.a;
    const int64_t t_k = up ? k - pl.a - 1 : pl.a - k - 1;      // where k's weight lies on this side
    double carry = 1.0;
    for (int64_t b0 = 0; b0 < len; b0 += TG_WAVE) {
        const bool in_side = b0 + lane < len;
        int64_t idx = -1;
        double x = in_side ? bt_ratio(up, pl.a, n, pl.r, b0 + lane, &idx) : 0.0;
#pragma unroll
        for (int o = 1; o < TG_WAVE; o <<= 1) {
            const double y = __shfl_up(x, o);
            if (lane >= o) x = y * x;
        }
        const double w = carry * x;
        if (by_index && t_k >= b0 && t_k < b0 + TG_WAVE && t_k < len) s.wk = __shfl(w, int(t_k - b0));
        const bool inc = in_side && (by_index ? (up ? idx >= k : idx <= k) : w <= thr);
        double sd = w, sn = inc ? w : 0.0;
#pragma unroll
        for (int o = 1; o < TG_WAVE; o <<= 1) {
            sd += __shfl_xor(sd, o);
            sn += __shfl_xor(sn, o);
        }
        s.den += sd;
        s.num += sn;
        carry = __shfl(w, TG_WAVE - 1);
        if (carry == 0.0) break;
    }
}

__device__ inline double wave_binom(const BtPlan& pl, int64_t k, int64_t n, int lane) {
    if (pl.decided) return pl.value;
    const bool near_up = !pl.low;
    WaveSums first = {0.0, 0.0, k == pl.a ? 1.0 : 0.0};
    wave_side(near_up, pl, k, n, true, 0.0, lane, first);
    const double thr = first.wk * TG_RERR;
    const bool anchor_in = (pl.low ? pl.a <= k : pl.a >= k) || ((pl.low ? pl.a >= pl.edge : pl.a <= pl.edge) && 1.0 <= thr);
    double num = anchor_in ? 1.0 : 0.0, den = 1.0;
    num += first.num;
    den += first.den;
    WaveSums second = {0.0, 0.0, 0.0};
    wave_side(!near_up, pl, k, n, false, thr, lane, second);
    num += second.num;
    den += second.den;
    const double v = num / den;
    return v < 1.0 ? v : 1.0;
}

// One wavefront per call, TG_WAVES calls per workgroup.  The lanes look through the segment table 64 rows at a time, in file order, and
// the lowest lane of the first 64 rows with a match wins; the table is read from global memory (every wave reads the same rows, which
// stay in cache), so there is no limit to it but the entry point's.  The wave then runs the call's two to four tests one after another.
// No LDS, no barrier, no atomics: a wave beyond the last call leaves at once.
__global__ __launch_bounds__(TG_THREADS) void k_tag_germline(const int32_t* __restrict__ ctg, const int64_t* __restrict__ pos,
                                                             const int64_t* __restrict__ depth, const double* __restrict__ freq, int64_t n_calls,
                                                             const int32_t* __restrict__ seg_chr, const int64_t* __restrict__ seg_start,
                                                             const int64_t* __restrict__ seg_end, const int64_t* __restrict__ seg_nmaj,
                                                             const int64_t* __restrict__ seg_nmin, int64_t S, double purity,
                                                             int32_t* __restrict__ seg, int32_t* __restrict__ status, double* __restrict__ af_out,
                                                             double* __restrict__ pv_out) {
    const int lane = threadIdx.x & (TG_WAVE - 1);
    const int64_t call = int64_t(blockIdx.x) * TG_WAVES + threadIdx.x / TG_WAVE;
    if (call >= n_calls) return;
    const int32_t c = ctg[call];
    const int64_t at = pos[call], n = depth[call];
    int64_t found = -1;
    for (int64_t b0 = 0; b0 < S; b0 += TG_WAVE) {
        const int64_t i = b0 + lane;
        const bool hit = i < S && seg_chr[i] == c && seg_start[i] <= at && at <= seg_end[i];
        const unsigned long long mask = __ballot(hit);
        if (mask) {
            found = b0 + (__ffsll(mask) - 1);
            break;
        }
    }
    double af[4] = {NAN, NAN, NAN, NAN}, pv[4] = {NAN, NAN, NAN, NAN};
    int32_t st = TG_FINE;
    if (found >= 0) {
        tg_fractions(purity, seg_nmaj[found], seg_nmin[found], af);
        const int64_t k = tg_successes(n, freq[call]);
        for (int j = 0; j < 4; ++j) {
            if (af[j] != af[j]) continue;
            const BtPlan pl = bt_plan(k, n, af[j]);
            if (pl.status != TG_FINE) {
                if (st == TG_FINE) st = pl.status;
                continue;
            }
            pv[j] = wave_binom(pl, k, n, lane);
        }
    }
    if (lane == 0) {
        seg[call] = int32_t(found);
        status[call] = st;
        for (int j = 0; j < 4; ++j) {
            af_out[call * 4 + j] = af[j];
            pv_out[call * 4 + j] = pv[j];
        }
    }
}

// the test rule alone, one wavefront per test
__global__ __launch_bounds__(TG_THREADS) void k_binom_two_sided(const int64_t* __restrict__ k, const int64_t* __restrict__ n, const double* __restrict__ p,
                                                                int64_t count, double* __restrict__ out, int32_t* __restrict__ status) {
    const int lane = threadIdx.x & (TG_WAVE - 1);
    const int64_t t = int64_t(blockIdx.x) * TG_WAVES + threadIdx.x / TG_WAVE;
    if (t >= count) return;
    const BtPlan pl = bt_plan(k[t], n[t], p[t]);
    const double v = pl.status == TG_FINE ? wave_binom(pl, k[t], n[t], lane) : NAN;
    if (lane == 0) {
        out[t] = v;
        status[t] = pl.status;
    }
}

struct TgContext : BatchCtx {};

// scipy's words for the first test that cannot be run
int report(const char* who, const int32_t* status, int64_t count, const int64_t* k, const int64_t* n, const double* p, const double* freq) {
    for (int64_t i = 0; i < count; ++i) {
        if (status[i] == TG_FINE) continue;
        const long long kk = k ? (long long)k[i] : (long long)tg_successes(n[i], freq[i]);
        if (status[i] == TG_BAD_N)
            set_error("%s: item %lld: n must be an integer not less than 1, but it is %lld", who, (long long)i, (long long)n[i]);
        else if (status[i] == TG_BAD_K && kk < 0)
            set_error("%s: item %lld: k must be an integer not less than 0, but it is %lld (n = %lld)", who, (long long)i, kk, (long long)n[i]);
        else if (status[i] == TG_BAD_K)
            set_error("%s: item %lld: k (%lld) must not be greater than n (%lld).", who, (long long)i, kk, (long long)n[i]);
        else if (p)
            set_error("%s: item %lld: p (%.17g) must be in range [0,1]", who, (long long)i, p[i]);
        else
            set_error("%s: item %lld: p must be in range [0,1]: the purity puts an expected allele fraction outside it", who, (long long)i);
        return CTO_EINVAL;
    }
    return CTO_OK;
}

}  // namespace

extern "C" int cto_tag_germline(const int32_t* ctg, const int64_t* pos, const int64_t* depth, const double* freq, int64_t n_calls,
                                const int32_t* seg_chr, const int64_t* seg_start, const int64_t* seg_end, const int64_t* seg_nmaj,
                                const int64_t* seg_nmin, int64_t S, double purity, int where, int32_t* seg, double* af, double* pv,
                                cto_tag_germline_stats* stats) try {
    if (stats) *stats = cto_tag_germline_stats{0, 0, 0, 0, 0.0};
    CTO_REQUIRE(n_calls >= 0 && S >= 0, CTO_EINVAL, "cto_tag_germline: %lld calls, %lld segments", (long long)n_calls, (long long)S);
    CTO_REQUIRE(where == 0 || where == 1, CTO_EINVAL, "cto_tag_germline: where is %d, not 0 (device) or 1 (host)", where);
    CTO_REQUIRE(n_calls == 0 || (ctg && pos && depth && freq && seg && af && pv), CTO_EINVAL, "cto_tag_germline: null array");
    CTO_REQUIRE(S == 0 || (seg_chr && seg_start && seg_end && seg_nmaj && seg_nmin), CTO_EINVAL, "cto_tag_germline: null array");
    CTO_REQUIRE(n_calls <= CTO_TAG_MAX_CALLS && S <= CTO_TAG_MAX_SEGMENTS, CTO_EUNSUPPORTED, "cto_tag_germline: %lld calls, %lld segments",
                (long long)n_calls, (long long)S);
    for (int64_t i = 0; i < n_calls; ++i)
        CTO_REQUIRE(depth[i] <= CTO_TAG_MAX_DEPTH, CTO_EUNSUPPORTED, "cto_tag_germline: call %lld has a depth of %lld", (long long)i, (long long)depth[i]);
    if (stats) { stats->n_calls = n_calls; stats->host_path = where; }
    if (n_calls == 0) return CTO_OK;
    std::vector<int32_t> status(size_t(n_calls), TG_FINE);

    if (where == 1) {
        const SegTable T = {seg_chr, seg_start, seg_end, seg_nmaj, seg_nmin, S};
        over_threads(size_t(n_calls), [&](size_t i) { host_call(T, purity, ctg[i], pos[i], depth[i], freq[i], &seg[i], &status[i], af + 4 * i, pv + 4 * i); });
    } else {
        int n_dev = 0;
        CTO_REQUIRE(hipGetDeviceCount(&n_dev) == hipSuccess && n_dev > 0, CTO_EHIP,
                    "cto_tag_germline: no HIP device (the host path is taken only when asked for)");
        // one upload: [pos | depth | freq | seg_start | seg_end | seg_nmaj | seg_nmin | ctg | seg_chr]; one download: [af | pv | seg | status]
        const size_t c8 = align16(size_t(n_calls) * 8), s8 = align16(size_t(S) * 8), c4 = align16(size_t(n_calls) * 4), s4 = align16(size_t(S) * 4);
        const size_t off_depth = c8, off_freq = 2 * c8, off_start = 3 * c8, off_end = off_start + s8, off_nmaj = off_end + s8, off_nmin = off_nmaj + s8,
                     off_ctg = off_nmin + s8, off_chr = off_ctg + c4, bytes_in = off_chr + s4;
        const size_t a32 = size_t(n_calls) * 32, off_pv = a32, off_seg = 2 * a32, off_status = off_seg + c4, bytes_out = off_status + c4;
        TgContext& X = process_wide<TgContext>();
        std::lock_guard<std::mutex> lock(X.mu);
        if (const int rc = X.open(bytes_in, bytes_out)) return rc;
        char* h = X.h_in.as<char>();
        memcpy(h, pos, size_t(n_calls) * 8);
        memcpy(h + off_depth, depth, size_t(n_calls) * 8);
        memcpy(h + off_freq, freq, size_t(n_calls) * 8);
        memcpy(h + off_ctg, ctg, size_t(n_calls) * 4);
        if (S) {
            memcpy(h + off_start, seg_start, size_t(S) * 8);
            memcpy(h + off_end, seg_end, size_t(S) * 8);
            memcpy(h + off_nmaj, seg_nmaj, size_t(S) * 8);
            memcpy(h + off_nmin, seg_nmin, size_t(S) * 8);
            memcpy(h + off_chr, seg_chr, size_t(S) * 4);
        }
        const char* din = X.d_in.as<char>();
        char* dout = X.d_out.as<char>();
        CTO_HIP(hipMemcpyAsync(X.d_in.p, h, bytes_in, hipMemcpyHostToDevice, X.stream));
        CTO_HIP(hipEventRecord(X.ev0, X.stream));
        const dim3 grid(uint32_t(cdiv(n_calls, TG_WAVES))), block(TG_THREADS);
        hipLaunchKernelGGL(k_tag_germline, grid, block, 0, X.stream, reinterpret_cast<const int32_t*>(din + off_ctg), reinterpret_cast<const int64_t*>(din),
                           reinterpret_cast<const int64_t*>(din + off_depth), reinterpret_cast<const double*>(din + off_freq), n_calls,
                           reinterpret_cast<const int32_t*>(din + off_chr), reinterpret_cast<const int64_t*>(din + off_start),
                           reinterpret_cast<const int64_t*>(din + off_end), reinterpret_cast<const int64_t*>(din + off_nmaj),
                           reinterpret_cast<const int64_t*>(din + off_nmin), S, purity, reinterpret_cast<int32_t*>(dout + off_seg),
                           reinterpret_cast<int32_t*>(dout + off_status), reinterpret_cast<double*>(dout), reinterpret_cast<double*>(dout + off_pv));
        CTO_HIP(hipGetLastError());
        CTO_HIP(hipEventRecord(X.ev1, X.stream));
        CTO_HIP(hipMemcpyAsync(X.h_out.p, X.d_out.p, bytes_out, hipMemcpyDeviceToHost, X.stream));
        CTO_HIP(record_and_wait(X.done, X.stream));
        if (stats) {
            float ms = 0.f;
            CTO_HIP(hipEventElapsedTime(&ms, X.ev0, X.ev1));
            stats->kernel_ms = ms;
        }
        const char* ho = X.h_out.as<char>();
        memcpy(af, ho, a32);
        memcpy(pv, ho + off_pv, a32);
        memcpy(seg, ho + off_seg, size_t(n_calls) * 4);
        memcpy(status.data(), ho + off_status, size_t(n_calls) * 4);
    }
    if (const int rc = report("cto_tag_germline", status.data(), n_calls, nullptr, depth, nullptr, freq)) return rc;
    if (stats)
        for (int64_t i = 0; i < n_calls; ++i) {
            stats->n_with_segment += seg[i] >= 0;
            for (int j = 0; j < 4; ++j) stats->n_tests += pv[4 * i + j] == pv[4 * i + j];
        }
    return CTO_OK;
}
CTO_CATCH("cto_tag_germline", int)

// the test rule alone on arrays of (k, n, p), on either path; for the tests
extern "C" int cto_binom_two_sided(const int64_t* k, const int64_t* n, const double* p, int64_t count, int where, double* out) try {
    CTO_REQUIRE(count >= 0 && (count == 0 || (k && n && p && out)), CTO_EINVAL, "cto_binom_two_sided: bad arguments");
    CTO_REQUIRE(where == 0 || where == 1, CTO_EINVAL, "cto_binom_two_sided: where is %d, not 0 (device) or 1 (host)", where);
    CTO_REQUIRE(count <= CTO_TAG_MAX_CALLS, CTO_EUNSUPPORTED, "cto_binom_two_sided: %lld tests", (long long)count);
    for (int64_t i = 0; i < count; ++i)
        CTO_REQUIRE(n[i] <= CTO_TAG_MAX_DEPTH, CTO_EUNSUPPORTED, "cto_binom_two_sided: test %lld has n = %lld", (long long)i, (long long)n[i]);
    if (count == 0) return CTO_OK;
    std::vector<int32_t> status(size_t(count), TG_FINE);
    if (where == 1) {
        over_threads(size_t(count), [&](size_t i) {
            const BtPlan pl = bt_plan(k[i], n[i], p[i]);
            status[i] = pl.status;
            out[i] = pl.status == TG_FINE ? host_binom(pl, k[i], n[i]) : NAN;
        });
    } else {
        int n_dev = 0;
        CTO_REQUIRE(hipGetDeviceCount(&n_dev) == hipSuccess && n_dev > 0, CTO_EHIP,
                    "cto_binom_two_sided: no HIP device (the host path is taken only when asked for)");
        const size_t c8 = align16(size_t(count) * 8), bytes_in = 3 * c8, bytes_out = c8 + size_t(count) * 4;
        TgContext& X = process_wide<TgContext>();
        std::lock_guard<std::mutex> lock(X.mu);
        if (const int rc = X.open(bytes_in, bytes_out)) return rc;
        char* h = X.h_in.as<char>();
        memcpy(h, k, size_t(count) * 8);
        memcpy(h + c8, n, size_t(count) * 8);
        memcpy(h + 2 * c8, p, size_t(count) * 8);
        const char* din = X.d_in.as<char>();
        char* dout = X.d_out.as<char>();
        CTO_HIP(hipMemcpyAsync(X.d_in.p, h, bytes_in, hipMemcpyHostToDevice, X.stream));
        const dim3 grid(uint32_t(cdiv(count, TG_WAVES))), block(TG_THREADS);
        hipLaunchKernelGGL(k_binom_two_sided, grid, block, 0, X.stream, reinterpret_cast<const int64_t*>(din), reinterpret_cast<const int64_t*>(din + c8),
                           reinterpret_cast<const double*>(din + 2 * c8), count, reinterpret_cast<double*>(dout), reinterpret_cast<int32_t*>(dout + c8));
        CTO_HIP(hipGetLastError());
        CTO_HIP(hipMemcpyAsync(X.h_out.p, X.d_out.p, bytes_out, hipMemcpyDeviceToHost, X.stream));
        CTO_HIP(record_and_wait(X.done, X.stream));
        memcpy(out, X.h_out.p, size_t(count) * 8);
        memcpy(status.data(), X.h_out.as<char>() + c8, size_t(count) * 4);
    }
    return report("cto_binom_two_sided", status.data(), count, k, n, p, nullptr);
}
CTO_CATCH("cto_binom_two_sided", int)
