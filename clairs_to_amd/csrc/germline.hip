// Germline genotypes of the Verdict step (src/verdict/predict_germline_genotypes.py of the reference, :70-154): per run of undecided probes
// the distance of every probe's mirrored BAF to the nearest of three sliding-window medians.  The kernel, the host path of the same call
// (the plain definition of the rules) and the entry point.  Compiled with -ffp-contract=off: a median of an even count is (a + b) / 2 and
// a distance |median - c[k]|, both as numpy computes them.
//
// The rules, over one run c[0..m) (DESIGN.md "Germline genotypes" derives them from the reference's index windows):
//   m <= 5: dist[k] = 1.   Otherwise L = min(m - 1, segment_length), H = L / 2 and
//     left    k >= L           median of c[k-L .. k-1]
//     right   k <  m - L       median of c[k+1 .. k+L]
//     middle  H <= k < m - H   median of c[k-H .. k-1] and c[k+1 .. k+H] together
//   dist[k] = the smallest |median - c[k]| over the defined ones, +inf when none is.
#include <algorithm>
#include <cmath>
#include <mutex>
#include <thread>
#include <vector>
#include "hip_buffers.h"

namespace {

using namespace cto;

constexpr int GG_THREADS = 256, GG_WAVES = GG_THREADS / 64;
constexpr int GG_TILE = CTO_GG_TILE;                           // probes of one run a workgroup takes
constexpr int GG_MAX_SEG = CTO_GG_MAX_SEGMENT;                 // the LDS copy holds the tile and GG_MAX_SEG values on either side
constexpr int GG_LDS = GG_TILE + 2 * GG_MAX_SEG;

struct GgTile { int64_t run_lo, run_hi, lo; };                 // probes [lo, min(lo + GG_TILE, run_hi)) of the run [run_lo, run_hi)

// ------------------------------------------------------------------------------------------------ kernel
__device__ inline double wave_max(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// Median of s[a0 .. a0+n0) and s[a1 .. a1+n1) taken together (1 <= n0 + n1 <= 64 * PER), by one wave: lane l holds the elements l, l + 64, ..
// and counts, for each, the window values below it (lt) and not above it (le), all PER of its elements in one pass over the window (an
// LDS read whose address is the same in every lane is a broadcast; four reads are in flight per step, or the loop would wait out one LDS
// latency per value).  In sorted order an element fills the ranks lt .. le - 1 together with its equals, so the value of rank r is that
// of ANY element with lt <= r < le: no tie-break is needed, and the two middle ranks reach every lane through a max over lanes that
// hold -inf unless they own the rank.  Every lane of the wave must call it.
constexpr int GG_PER_LANE = (GG_MAX_SEG + 63) / 64;

template <int PER>
__device__ inline double wave_median_of(const double* s, int a0, int n0, int a1, int n1, int lane) {
    const int n = n0 + n1, r_lo = (n - 1) >> 1, r_hi = n >> 1;
    double v[PER];
    int lt[PER], le[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int e = lane + 64 * i;
        v[i] = e < n ? s[e < n0 ? a0 + e : a1 + e - n0] : INFINITY;
        lt[i] = le[i] = 0;
    }
    auto count = [&](double u) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            lt[i] += u < v[i] ? 1 : 0;
            le[i] += u <= v[i] ? 1 : 0;
        }
    };
    auto pass = [&](const double* w, int cnt) {
        int j = 0;
        for (; j + 4 <= cnt; j += 4) {
            const double u0 = w[j], u1 = w[j + 1], u2 = w[j + 2], u3 = w[j + 3];
            count(u0);
            count(u1);
            count(u2);
            count(u3);
        }
        for (; j < cnt; ++j) count(w[j]);
    };
    pass(s + a0, n0);
    pass(s + a1, n1);
    double lo = -INFINITY, hi = -INFINITY;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const bool mine = lane + 64 * i < n;
        if (mine && lt[i] <= r_lo && r_lo < le[i]) lo = v[i];
        if (mine && lt[i] <= r_hi && r_hi < le[i]) hi = v[i];
    }
    lo = wave_max(lo);
    hi = wave_max(hi);
    return (n & 1) ? hi : (lo + hi) / 2;
}

__device__ inline double wave_median(const double* s, int a0, int n0, int a1, int n1, int lane) {
    static_assert(GG_PER_LANE == 4, "one case per element count of a lane");
    const int per = (n0 + n1 + 63) >> 6;                       // the same in every lane
    if (per <= 1) return wave_median_of<1>(s, a0, n0, a1, n1, lane);
    if (per == 2) return wave_median_of<2>(s, a0, n0, a1, n1, lane);
    if (per == 3) return wave_median_of<3>(s, a0, n0, a1, n1, lane);
    return wave_median_of<4>(s, a0, n0, a1, n1, lane);
}

// One workgroup per tile; a tile lies within one run.  LDS holds c[lo - L .. lo + tile + L), clipped to the run (what lies outside is
// written as 0 and never read: the three conditions above keep every window inside the run).  Waves take the tile's probes in turn; the
// conditions are the same in every lane of a wave.
__global__ __launch_bounds__(GG_THREADS) void k_germline_dist(const GgTile* __restrict__ tiles, const double* __restrict__ c, int segment_length,
                                                              double* __restrict__ dist) {
    __shared__ double s[GG_LDS];
    const GgTile t = tiles[blockIdx.x];
    const int64_t m = t.run_hi - t.run_lo;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int n_here = int(min((long long)GG_TILE, (long long)(t.run_hi - t.lo)));
    if (m <= 5) {                                              // :149-150
        if (tid < n_here) dist[t.lo + tid] = 1.0;
        return;
    }
    const int L = int(min((long long)(m - 1), (long long)segment_length)), H = L >> 1;     // L <= GG_MAX_SEG (the entry point's gate)
    const int64_t g0 = t.lo - L;
    for (int j = tid; j < n_here + 2 * L; j += GG_THREADS) {
        const int64_t g = g0 + j;
        s[j] = (g >= t.run_lo && g < t.run_hi) ? c[g] : 0.0;
    }
    __syncthreads();
    for (int p = wave; p < n_here; p += GG_WAVES) {
        const int64_t k = t.lo + p - t.run_lo;
        const int q = p + L;                                   // the probe's place in s
        const double x = s[q];
        double best = INFINITY;
        if (k >= L) best = fmin(best, fabs(wave_median(s, q - L, L, 0, 0, lane) - x));
        if (k < m - L) best = fmin(best, fabs(wave_median(s, q + 1, L, 0, 0, lane) - x));
        if (k >= H && k < m - H) best = fmin(best, fabs(wave_median(s, q - H, H, q + 1, H, lane) - x));
        if (lane == 0) dist[t.lo + p] = best;
    }
}

// ------------------------------------------------------------------------------------------------ host path
double median_of(std::vector<double>& w) {                     // np.median of a non-empty list without NaN
    const size_t n = w.size(), h = n / 2;
    std::nth_element(w.begin(), w.begin() + h, w.end());
    const double hi = w[h];
    if (n & 1) return hi;
    return (*std::max_element(w.begin(), w.begin() + h) + hi) / 2;
}

void run_on_host(const double* r, int64_t m, int segment_length, int64_t k0, int64_t k1, double* out) {      // probes [k0, k1) of the run r[0..m)
    if (m <= 5) {
        std::fill(out + k0, out + k1, 1.0);
        return;
    }
    const int64_t L = std::min<int64_t>(m - 1, segment_length), H = L / 2;
    std::vector<double> w;
    for (int64_t k = k0; k < k1; ++k) {
        double best = INFINITY;
        if (k >= L) {
            w.assign(r + k - L, r + k);
            best = std::min(best, std::fabs(median_of(w) - r[k]));
        }
        if (k < m - L) {
            w.assign(r + k + 1, r + k + L + 1);
            best = std::min(best, std::fabs(median_of(w) - r[k]));
        }
        if (k >= H && k < m - H) {
            w.assign(r + k - H, r + k);
            w.insert(w.end(), r + k + 1, r + k + H + 1);
            best = std::min(best, std::fabs(median_of(w) - r[k]));
        }
        out[k] = best;
    }
}

void all_on_host(const double* c, const int64_t* run_off, int64_t n_runs, int segment_length, double* dist) {
    struct Piece { int64_t run, k0, k1; };
    std::vector<Piece> pieces;                                 // at most 4096 probes each, so that one long run spreads over the threads
    for (int64_t r = 0; r < n_runs; ++r)
        for (int64_t k = 0, m = run_off[r + 1] - run_off[r]; k < m; k += 4096) pieces.push_back({r, k, std::min<int64_t>(k + 4096, m)});
    const unsigned hw = std::thread::hardware_concurrency();
    const size_t n_threads = std::max<size_t>(1, std::min<size_t>({size_t(hw ? hw : 1), size_t(16), pieces.size() / 4}));
    auto work = [&](size_t t) {
        for (size_t i = t; i < pieces.size(); i += n_threads) {
            const Piece& p = pieces[i];
            run_on_host(c + run_off[p.run], run_off[p.run + 1] - run_off[p.run], segment_length, p.k0, p.k1, dist + run_off[p.run]);
        }
    };
    std::vector<std::thread> threads;
    for (size_t t = 1; t < n_threads; ++t) threads.emplace_back(work, t);
    work(0);
    for (auto& th : threads) th.join();
}

struct GgContext : BatchCtx {};                                // the device side, one call at a time: the buffers outlive the calls

}  // namespace

extern "C" int cto_germline_window_dist(const double* c, const int64_t* run_off, int64_t n_runs, int segment_length, int force_host, double* dist,
                                        cto_germline_stats* stats) try {
    if (stats) *stats = cto_germline_stats{0, 0, 0, 0.0};
    CTO_REQUIRE(n_runs >= 0 && run_off, CTO_EINVAL, "cto_germline_window_dist: bad arguments");
    CTO_REQUIRE(segment_length >= 2, CTO_EINVAL, "cto_germline_window_dist: segment_length %d is below 2 (the reference raises there)", segment_length);
    CTO_REQUIRE(run_off[0] == 0, CTO_EINVAL, "cto_germline_window_dist: run_off[0] is %lld, not 0", (long long)run_off[0]);
    for (int64_t r = 0; r < n_runs; ++r)
        CTO_REQUIRE(run_off[r + 1] >= run_off[r], CTO_EINVAL, "cto_germline_window_dist: the offsets do not ascend at run %lld", (long long)r);
    const int64_t n = run_off[n_runs];
    CTO_REQUIRE(n == 0 || (c && dist), CTO_EINVAL, "cto_germline_window_dist: null array");
    for (int64_t i = 0; i < n; ++i) CTO_REQUIRE(!std::isnan(c[i]), CTO_EINVAL, "cto_germline_window_dist: value %lld is NaN", (long long)i);
    if (stats) { stats->n_runs = n_runs; stats->n_probes = n; }
    if (n == 0) return CTO_OK;

    if (force_host || segment_length > GG_MAX_SEG) {
        all_on_host(c, run_off, n_runs, segment_length, dist);
        if (stats) stats->host_path = 1;
        return CTO_OK;
    }
    int n_dev = 0;
    CTO_REQUIRE(hipGetDeviceCount(&n_dev) == hipSuccess && n_dev > 0, CTO_EHIP,
                "cto_germline_window_dist: no HIP device (the host path is taken only when asked for)");

    std::vector<GgTile> tiles;
    for (int64_t r = 0; r < n_runs; ++r)
        for (int64_t lo = run_off[r]; lo < run_off[r + 1]; lo += GG_TILE) tiles.push_back({run_off[r], run_off[r + 1], lo});
    CTO_REQUIRE(tiles.size() < 0x7fffffffu, CTO_EUNSUPPORTED, "cto_germline_window_dist: %zu tiles in one call", tiles.size());

    // one upload: [tiles | c]
    const size_t off_c = align16(tiles.size() * sizeof(GgTile)), bytes_in = off_c + size_t(n) * 8, bytes_out = size_t(n) * 8;
    GgContext& X = process_wide<GgContext>();
    std::lock_guard<std::mutex> lock(X.mu);
    if (const int rc = X.open(bytes_in, bytes_out)) return rc;
    char* h = X.h_in.as<char>();
    memcpy(h, tiles.data(), tiles.size() * sizeof(GgTile));
    memcpy(h + off_c, c, size_t(n) * 8);
    char* d = X.d_in.as<char>();
    CTO_HIP(hipMemcpyAsync(d, h, bytes_in, hipMemcpyHostToDevice, X.stream));
    CTO_HIP(hipEventRecord(X.ev0, X.stream));
    hipLaunchKernelGGL(k_germline_dist, dim3(uint32_t(tiles.size())), dim3(GG_THREADS), 0, X.stream, reinterpret_cast<const GgTile*>(d),
                       reinterpret_cast<const double*>(d + off_c), segment_length, X.d_out.as<double>());
    CTO_HIP(hipGetLastError());
    CTO_HIP(hipEventRecord(X.ev1, X.stream));
    CTO_HIP(hipMemcpyAsync(X.h_out.p, X.d_out.p, bytes_out, hipMemcpyDeviceToHost, X.stream));
    CTO_HIP(record_and_wait(X.done, X.stream));
    if (stats) {
        float ms = 0.f;
        CTO_HIP(hipEventElapsedTime(&ms, X.ev0, X.ev1));
        stats->kernel_ms = ms;
    }
    memcpy(dist, X.h_out.p, bytes_out);
    return CTO_OK;
}
CTO_CATCH("cto_germline_window_dist", int)
