// ASPCF, the segmentation step of the Verdict chain (src/verdict/aspcf.py of the reference): the penalised least-squares recurrence of
// aspcfpart over many independent windows (the kernel, the host path of the same call, the entry point), and two host-only calls, the
// running median of medianFilter and the single-track recurrence of exactPcf.  Compiled with -ffp-contract=off: every sum, product and
// division below is the one numpy does, in its order.  DESIGN.md "ASPCF" derives the rules from the reference's slices.
//
// The rules, over one window a[0..N), b[0..N) with divisors v1, v2 (N < 2 * kmin: no fit, all zeros):
//   i1, i2 = the sums of the first kmin values, q1, q2 = the sums of their squares (plain products);
//   best[kmin-1] = (q1 - i1 * (i1 / kmin)) / v1 + (q2 - i2 * (i2 / kmin)) / v2.
//   For n = kmin+1 .. N: every slot s in [kmin, n) does S1[s] += a[n-1], K1[s] += sq(a[n-1]) (and S2, K2 with b);
//     t1 = (S1[kmin] + i1) / n, tot = ((K1[kmin] + q1) - n * sq(t1)) / v1 + (the same of track 2);
//     n < 2 * kmin: best[n-1] = tot, split[n-1] = 0;
//     otherwise C[s] = (best[s-1] + (K1[s] - S1[s] * (S1[s] / (n-s))) / v1) + (K2[s] - S2[s] * (S2[s] / (n-s))) / v2 for s in [kmin, n-kmin],
//       m = the first arg-min of C, q = m - 1 (the reference reads the slot BEFORE its arg-min), cost = (q >= kmin ? C[q] : 0) + gamma;
//       tot < cost: q = 0, cost = tot;  best[n-1] = cost, split[n-1] = q.
// sq() is libm's pow(x, 2.0), which is what a numpy scalar ** 2 calls and not always x * x.  Everything that depends on a window's
// prefix alone (the squares, i1 .. q2, tot[n]) is prepared once by the host code of the call and read by both paths: the kernel never
// squares a value, and it sees the numbers the host path sees.
#include <algorithm>
#include <climits>
#include <cmath>
#include <mutex>
#include <thread>
#include <vector>
#include "hip_buffers.h"

namespace {

using namespace cto;

constexpr int AS_THREADS = 256, AS_WAVES = AS_THREADS / 64;
constexpr int AS_MAX_WINDOW = CTO_ASPCF_MAX_WINDOW;
constexpr int AS_PER = (AS_MAX_WINDOW + AS_THREADS - 1) / AS_THREADS;    // slots of one thread

struct AsWindow { int64_t lo, out; int32_t n, pad; double v1, v2; };     // values [lo, lo + n) of the chromosome; `out` = its place in the
                                                                         // concatenated per-window arrays (tot, best_cost, best_split)

// the exponent is read at run time: a literal 2.0 would let the compiler turn the call into x * x
double sq(double x) {
    static volatile double two = 2.0;
    return std::pow(x, two);
}

// ------------------------------------------------------------------------------------------------ prepared per window
// tot[i] for a window of n values: 0 below kmin - 1, the initial cost at kmin - 1, tot of step i + 1 above it.  best[i] = tot[i] for
// i < 2 * kmin - 1.  n >= 2 * kmin.
void prepare_window(const double* a, const double* b, const double* sa, const double* sb, int n, int kmin, double v1, double v2, double* tot) {
    double i1 = 0, i2 = 0, q1 = 0, q2 = 0;
    for (int i = 0; i < kmin; ++i) {
        i1 += a[i];
        q1 += a[i] * a[i];
        i2 += b[i];
        q2 += b[i] * b[i];
    }
    std::fill(tot, tot + kmin - 1, 0.0);
    tot[kmin - 1] = (q1 - i1 * (i1 / kmin)) / v1 + (q2 - i2 * (i2 / kmin)) / v2;
    double s1 = 0, k1 = 0, s2 = 0, k2 = 0;                       // the slot kmin
    for (int m = kmin + 1; m <= n; ++m) {
        s1 += a[m - 1];
        k1 += sa[m - 1];
        s2 += b[m - 1];
        k2 += sb[m - 1];
        const double t1 = (s1 + i1) / m, t2 = (s2 + i2) / m;
        tot[m - 1] = ((k1 + q1) - m * sq(t1)) / v1 + ((k2 + q2) - m * sq(t2)) / v2;
    }
}

// ------------------------------------------------------------------------------------------------ kernel
struct Cand { double c; int s; };

__device__ inline Cand better(Cand x, Cand y) { return (y.c < x.c || (y.c == x.c && y.s < x.s)) ? y : x; }

__device__ inline Cand wave_argmin(Cand x) {
    for (int o = 32; o > 0; o >>= 1) {
        Cand y;
        y.c = __shfl_xor(x.c, o);
        y.s = __shfl_xor(x.s, o);
        x = better(x, y);
    }
    return x;
}

// One workgroup per window.  Slot kmin + tid + 256 j is the thread's j-th; its sums and best[s-1] stay in registers for the whole window.
// A step: update the live slots, publish the candidates' C to LDS, arg-min by wave shuffles then over the waves' results in LDS, one
// barrier; then EVERY thread finishes the step (the same four partial results, the same C[m-1]), so that the thread that owns slot n
// keeps best[n-1] for it without another barrier.  C and the partial results are double-buffered by step parity: a thread that writes
// them at step n + 1 has passed the barrier of step n, which every thread reaches only after its reads of step n - 1.
__global__ __launch_bounds__(AS_THREADS) void k_aspcf_windows(const AsWindow* __restrict__ wins, const double* __restrict__ y1, const double* __restrict__ y2,
                                                              const double* __restrict__ sq1, const double* __restrict__ sq2,
                                                              const double* __restrict__ tot_all, int kmin, double gamma,
                                                              double* __restrict__ best_all, int32_t* __restrict__ split_all) {
    __shared__ double s_a[AS_MAX_WINDOW], s_b[AS_MAX_WINDOW], s_sa[AS_MAX_WINDOW], s_sb[AS_MAX_WINDOW], s_tot[AS_MAX_WINDOW];
    __shared__ double s_c[2][AS_MAX_WINDOW], s_best[AS_MAX_WINDOW];
    __shared__ int s_split[AS_MAX_WINDOW];
    __shared__ double s_pc[2][AS_WAVES];
    __shared__ int s_ps[2][AS_WAVES];

    const AsWindow w = wins[blockIdx.x];
    const int N = w.n, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (N < 2 * kmin) {                                          // no fit
        for (int i = tid; i < N; i += AS_THREADS) {
            best_all[w.out + i] = 0.0;
            split_all[w.out + i] = 0;
        }
        return;
    }
    for (int i = tid; i < N; i += AS_THREADS) {
        s_a[i] = y1[w.lo + i];
        s_b[i] = y2[w.lo + i];
        s_sa[i] = sq1[w.lo + i];
        s_sb[i] = sq2[w.lo + i];
        const double t = tot_all[w.out + i];
        s_tot[i] = t;
        s_best[i] = i < 2 * kmin - 1 ? t : 0.0;
        s_split[i] = 0;
    }
    __syncthreads();

    double S1[AS_PER], K1[AS_PER], S2[AS_PER], K2[AS_PER], prev[AS_PER];
#pragma unroll
    for (int j = 0; j < AS_PER; ++j) {
        const int s = kmin + tid + AS_THREADS * j;
        S1[j] = K1[j] = S2[j] = K2[j] = 0.0;
        prev[j] = (s < 2 * kmin && s < N) ? s_tot[s - 1] : 0.0;  // best[s-1] of the steps without candidates; the others are kept as they are found
    }
    const double v1 = w.v1, v2 = w.v2;

    for (int n = kmin + 1; n <= N; ++n) {
        const double xa = s_a[n - 1], xb = s_b[n - 1], xsa = s_sa[n - 1], xsb = s_sb[n - 1];
        const bool fit = n >= 2 * kmin;                          // the same in every thread
        const int buf = n & 1;
        Cand mine{INFINITY, INT_MAX};
#pragma unroll
        for (int j = 0; j < AS_PER; ++j) {
            const int s = kmin + tid + AS_THREADS * j;
            if (s < n) {
                S1[j] += xa;
                K1[j] += xsa;
                S2[j] += xb;
                K2[j] += xsb;
                if (fit && s <= n - kmin) {
                    const double cnt = double(n - s);
                    const double c = (prev[j] + (K1[j] - S1[j] * (S1[j] / cnt)) / v1) + (K2[j] - S2[j] * (S2[j] / cnt)) / v2;
                    s_c[buf][s - kmin] = c;
                    if (c < mine.c || mine.s == INT_MAX) mine = Cand{c, s};     // slots ascend with j: the first of equal values stays
                }
            }
        }
        if (!fit) continue;
        mine = wave_argmin(mine);
        if (lane == 0) {
            s_pc[buf][wave] = mine.c;
            s_ps[buf][wave] = mine.s;
        }
        __syncthreads();
        Cand m{s_pc[buf][0], s_ps[buf][0]};
#pragma unroll
        for (int k = 1; k < AS_WAVES; ++k) m = better(m, Cand{s_pc[buf][k], s_ps[buf][k]});
        int q = m.s - 1;
        double cost = (q >= kmin ? s_c[buf][q - kmin] : 0.0) + gamma;
        const double t = s_tot[n - 1];
        if (t < cost) {
            q = 0;
            cost = t;
        }
        if (tid == 0) {
            s_best[n - 1] = cost;
            s_split[n - 1] = q;
        }
#pragma unroll
        for (int j = 0; j < AS_PER; ++j)
            if (kmin + tid + AS_THREADS * j == n) prev[j] = cost;       // best[s-1] of the slot s = n
    }
    __syncthreads();
    for (int i = tid; i < N; i += AS_THREADS) {
        best_all[w.out + i] = s_best[i];
        split_all[w.out + i] = s_split[i];
    }
}

// ------------------------------------------------------------------------------------------------ host path
void window_on_host(const double* a, const double* b, const double* sa, const double* sb, const double* tot, int N, int kmin, double v1, double v2,
                    double gamma, double* best, int32_t* split) {
    std::fill(best, best + N, 0.0);
    std::fill(split, split + N, 0);
    if (N < 2 * kmin) return;
    std::copy(tot, tot + 2 * kmin - 1, best);
    std::vector<double> S1(N, 0.0), K1(N, 0.0), S2(N, 0.0), K2(N, 0.0), Cs(N, 0.0);
    for (int n = kmin + 1; n <= N; ++n) {
        for (int s = kmin; s < n; ++s) {
            S1[s] += a[n - 1];
            K1[s] += sa[n - 1];
            S2[s] += b[n - 1];
            K2[s] += sb[n - 1];
        }
        if (n < 2 * kmin) continue;
        int m = kmin;
        for (int s = kmin; s <= n - kmin; ++s) {
            const double cnt = double(n - s);
            Cs[s] = (best[s - 1] + (K1[s] - S1[s] * (S1[s] / cnt)) / v1) + (K2[s] - S2[s] * (S2[s] / cnt)) / v2;
            if (Cs[s] < Cs[m]) m = s;
        }
        int q = m - 1;
        double cost = (q >= kmin ? Cs[q] : 0.0) + gamma;
        if (tot[n - 1] < cost) {
            q = 0;
            cost = tot[n - 1];
        }
        best[n - 1] = cost;
        split[n - 1] = q;
    }
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

struct AsContext : BatchCtx {};                                  // the device side, one call at a time: the buffers outlive the calls

}  // namespace

extern "C" int cto_aspcf_windows(const double* y1, const double* y2, int64_t n, const int64_t* win_lo, const int64_t* win_hi, int64_t n_win,
                                 const double* v1, const double* v2, int kmin, double gamma, int force_host, int32_t* best_split,
                                 double* best_cost, cto_aspcf_stats* stats) try {
    if (stats) *stats = cto_aspcf_stats{0, 0, 0, 0.0};
    CTO_REQUIRE(n >= 0 && n_win >= 0, CTO_EINVAL, "cto_aspcf_windows: bad arguments");
    CTO_REQUIRE(kmin >= 1, CTO_EINVAL, "cto_aspcf_windows: kmin %d is below 1", kmin);
    CTO_REQUIRE(!std::isnan(gamma), CTO_EINVAL, "cto_aspcf_windows: gamma is NaN");
    CTO_REQUIRE(n == 0 || (y1 && y2), CTO_EINVAL, "cto_aspcf_windows: null array");
    CTO_REQUIRE(n_win == 0 || (win_lo && win_hi && v1 && v2), CTO_EINVAL, "cto_aspcf_windows: null window array");
    for (int64_t i = 0; i < n; ++i)
        CTO_REQUIRE(std::isfinite(y1[i]) && std::isfinite(y2[i]), CTO_EINVAL, "cto_aspcf_windows: value %lld is NaN or infinite", (long long)i);
    std::vector<AsWindow> wins(size_t(n_win), AsWindow{});
    int64_t total = 0;
    for (int64_t k = 0; k < n_win; ++k) {
        const int64_t len = win_hi[k] - win_lo[k];
        CTO_REQUIRE(win_lo[k] >= 0 && len >= 0 && win_hi[k] <= n, CTO_EINVAL, "cto_aspcf_windows: window %lld [%lld, %lld) is not within the %lld values",
                    (long long)k, (long long)win_lo[k], (long long)win_hi[k], (long long)n);
        CTO_REQUIRE(len <= AS_MAX_WINDOW, CTO_EINVAL, "cto_aspcf_windows: window %lld holds %lld values, more than %d", (long long)k, (long long)len,
                    AS_MAX_WINDOW);
        CTO_REQUIRE(v1[k] > 0 && v2[k] > 0 && std::isfinite(v1[k]) && std::isfinite(v2[k]), CTO_EINVAL,
                    "cto_aspcf_windows: the divisors of window %lld (%g, %g) are not positive numbers", (long long)k, v1[k], v2[k]);
        wins[size_t(k)] = AsWindow{win_lo[k], total, int32_t(len), 0, v1[k], v2[k]};
        total += len;
    }
    CTO_REQUIRE(total == 0 || best_split, CTO_EINVAL, "cto_aspcf_windows: null output");
    if (stats) { stats->n_windows = n_win; stats->n_values = total; }
    if (total == 0) return CTO_OK;

    // what both paths read: the squares, once per value, and tot per window
    std::vector<double> sq1(size_t(n), 0.0), sq2(size_t(n), 0.0), tot(size_t(total), 0.0);
    over_threads(size_t((n + 16383) / 16384), [&](size_t piece) {
        for (int64_t i = int64_t(piece) * 16384, end = std::min<int64_t>(n, i + 16384); i < end; ++i) {
            sq1[size_t(i)] = sq(y1[i]);
            sq2[size_t(i)] = sq(y2[i]);
        }
    });
    over_threads(wins.size(), [&](size_t k) {
        const AsWindow& w = wins[k];
        if (w.n >= 2 * kmin) prepare_window(y1 + w.lo, y2 + w.lo, sq1.data() + w.lo, sq2.data() + w.lo, w.n, kmin, w.v1, w.v2, tot.data() + w.out);
    });

    if (force_host) {
        std::vector<double> cost_here(best_cost ? 0 : size_t(total));
        double* cost = best_cost ? best_cost : cost_here.data();
        over_threads(wins.size(), [&](size_t k) {
            const AsWindow& w = wins[k];
            window_on_host(y1 + w.lo, y2 + w.lo, sq1.data() + w.lo, sq2.data() + w.lo, tot.data() + w.out, w.n, kmin, w.v1, w.v2, gamma, cost + w.out,
                           best_split + w.out);
        });
        if (stats) stats->host_path = 1;
        return CTO_OK;
    }
    int n_dev = 0;
    CTO_REQUIRE(hipGetDeviceCount(&n_dev) == hipSuccess && n_dev > 0, CTO_EHIP,
                "cto_aspcf_windows: no HIP device (the host path is taken only when asked for)");
    CTO_REQUIRE(wins.size() < 0x7fffffffu, CTO_EUNSUPPORTED, "cto_aspcf_windows: %zu windows in one call", wins.size());

    // one upload: [windows | y1 | y2 | sq1 | sq2 | tot]; one download: [best_cost | best_split]
    const size_t bytes_w = align16(wins.size() * sizeof(AsWindow)), bytes_y = align16(size_t(n) * 8), bytes_t = align16(size_t(total) * 8);
    const size_t off_y1 = bytes_w, off_y2 = off_y1 + bytes_y, off_s1 = off_y2 + bytes_y, off_s2 = off_s1 + bytes_y, off_tot = off_s2 + bytes_y;
    const size_t bytes_in = off_tot + bytes_t, bytes_out = bytes_t + size_t(total) * 4;
    AsContext& X = process_wide<AsContext>();
    std::lock_guard<std::mutex> lock(X.mu);
    if (const int rc = X.open(bytes_in, bytes_out)) return rc;
    char* h = X.h_in.as<char>();
    memcpy(h, wins.data(), wins.size() * sizeof(AsWindow));
    memcpy(h + off_y1, y1, size_t(n) * 8);
    memcpy(h + off_y2, y2, size_t(n) * 8);
    memcpy(h + off_s1, sq1.data(), size_t(n) * 8);
    memcpy(h + off_s2, sq2.data(), size_t(n) * 8);
    memcpy(h + off_tot, tot.data(), size_t(total) * 8);
    char* d = X.d_in.as<char>();
    char* d_out = X.d_out.as<char>();
    CTO_HIP(hipMemcpyAsync(d, h, bytes_in, hipMemcpyHostToDevice, X.stream));
    CTO_HIP(hipEventRecord(X.ev0, X.stream));
    hipLaunchKernelGGL(k_aspcf_windows, dim3(uint32_t(wins.size())), dim3(AS_THREADS), 0, X.stream, reinterpret_cast<const AsWindow*>(d),
                       reinterpret_cast<const double*>(d + off_y1), reinterpret_cast<const double*>(d + off_y2),
                       reinterpret_cast<const double*>(d + off_s1), reinterpret_cast<const double*>(d + off_s2),
                       reinterpret_cast<const double*>(d + off_tot), kmin, gamma, reinterpret_cast<double*>(d_out),
                       reinterpret_cast<int32_t*>(d_out + bytes_t));
    CTO_HIP(hipGetLastError());
    CTO_HIP(hipEventRecord(X.ev1, X.stream));
    CTO_HIP(hipMemcpyAsync(X.h_out.p, X.d_out.p, bytes_out, hipMemcpyDeviceToHost, X.stream));
    CTO_HIP(record_and_wait(X.done, X.stream));
    if (stats) {
        float ms = 0.f;
        CTO_HIP(hipEventElapsedTime(&ms, X.ev0, X.ev1));
        stats->kernel_ms = ms;
    }
    if (best_cost) memcpy(best_cost, X.h_out.p, size_t(total) * 8);
    memcpy(best_split, X.h_out.as<char>() + bytes_t, size_t(total) * 4);
    return CTO_OK;
}
CTO_CATCH("cto_aspcf_windows", int)

// the squares as both paths read them (for the tests: libm's pow is an assumption about the machine)
extern "C" int cto_aspcf_squares(const double* x, int64_t n, double* out) try {
    CTO_REQUIRE(n >= 0 && (n == 0 || (x && out)), CTO_EINVAL, "cto_aspcf_squares: bad arguments");
    for (int64_t i = 0; i < n; ++i) out[i] = sq(x[i]);
    return CTO_OK;
}
CTO_CATCH("cto_aspcf_squares", int)

// medianFilter of the reference: scipy.ndimage.median_filter(x, size = width, mode = 'reflect') with an odd width - every output is
// one of the inputs, the middle rank of the window x[i - h .. i + h] with indices beyond the ends reflected (-1 -> 0, n -> n - 1).
extern "C" int cto_running_median(const double* x, int64_t n, int k, double* out) try {
    CTO_REQUIRE(n >= 0 && k >= 0 && (n == 0 || (x && out)), CTO_EINVAL, "cto_running_median: bad arguments");
    for (int64_t i = 0; i < n; ++i) CTO_REQUIRE(!std::isnan(x[i]), CTO_EINVAL, "cto_running_median: value %lld is NaN", (long long)i);
    if (n == 0) return CTO_OK;
    int64_t width = 2 * int64_t(k) + 1;
    if (width > n) width = (n % 2 == 0) ? n - 1 : n;
    const int64_t h = width / 2;                                 // h < n: one reflection is enough
    over_threads(size_t((n + 4095) / 4096), [&](size_t piece) {
        std::vector<double> w{};
        w.resize(size_t(width));
        for (int64_t i = int64_t(piece) * 4096, end = std::min<int64_t>(n, i + 4096); i < end; ++i) {
            for (int64_t j = i - h; j <= i + h; ++j) w[size_t(j - i + h)] = x[j < 0 ? -j - 1 : j >= n ? 2 * n - 1 - j : j];
            std::nth_element(w.begin(), w.begin() + h, w.end());
            out[i] = w[size_t(h)];
        }
    });
    return CTO_OK;
}
CTO_CATCH("cto_running_median", int)

// exactPcf of the reference, the single-track form: no divisors, gamma inside C before the arg-min, and again the slot before the
// arg-min: cost = q >= kmin ? C[q] : 0, aver = q >= kmin ? S[q] / (n - q) : 0.  yhat is filled from the averages along the traceback.
extern "C" int cto_exact_pcf(const double* y, int64_t n, int kmin, double gamma, double* yhat) try {
    CTO_REQUIRE(kmin >= 1, CTO_EINVAL, "cto_exact_pcf: kmin %d is below 1", kmin);
    CTO_REQUIRE(y && yhat && n >= 2 * int64_t(kmin), CTO_EINVAL, "cto_exact_pcf: %lld values are fewer than 2 * kmin (the caller takes their mean)", (long long)n);
    CTO_REQUIRE(n < INT_MAX, CTO_EUNSUPPORTED, "cto_exact_pcf: %lld values", (long long)n);
    for (int64_t i = 0; i < n; ++i) CTO_REQUIRE(std::isfinite(y[i]), CTO_EINVAL, "cto_exact_pcf: value %lld is NaN or infinite", (long long)i);
    const int N = int(n);
    double i0 = 0, q0 = 0;
    for (int i = 0; i < kmin; ++i) {
        i0 += y[i];
        q0 += y[i] * y[i];
    }
    std::vector<double> best(size_t(N), 0.0), aver(size_t(N), 0.0), S(size_t(N), 0.0), K(size_t(N), 0.0), Cs(size_t(N), 0.0);
    std::vector<int> split(size_t(N), 0);
    aver[kmin - 1] = i0 / kmin;
    best[kmin - 1] = q0 - i0 * aver[kmin - 1];
    for (int m = kmin + 1; m <= N; ++m) {
        const double x = y[m - 1], x2 = sq(x);
        for (int s = kmin; s < m; ++s) {
            S[s] += x;
            K[s] += x2;
        }
        const double t_aver = (S[kmin] + i0) / m, t_cost = (K[kmin] + q0) - m * sq(t_aver);
        if (m < 2 * kmin) {
            aver[m - 1] = t_aver;
            best[m - 1] = t_cost;
            continue;
        }
        int a = kmin;
        for (int s = kmin; s <= m - kmin; ++s) {
            Cs[s] = ((best[s - 1] + K[s]) - S[s] * (S[s] / double(m - s))) + gamma;
            if (Cs[s] < Cs[a]) a = s;
        }
        int q = a - 1;
        double cost = q >= kmin ? Cs[q] : 0.0, av = q >= kmin ? S[q] / double(m - q) : 0.0;
        if (t_cost < cost) {
            q = 0;
            cost = t_cost;
            av = t_aver;
        }
        best[m - 1] = cost;
        aver[m - 1] = av;
        split[m - 1] = q;
    }
    for (int m = N; m > 0; m = split[m - 1]) std::fill(yhat + split[m - 1], yhat + m, aver[m - 1]);
    return CTO_OK;
}
CTO_CATCH("cto_exact_pcf", int)
