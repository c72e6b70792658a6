// The purity/ploidy grid of run_ascat, the fit step of the Verdict chain (create_distance_matrix, src/verdict/run_ascat.py:31-60 of the
// reference): the distance of every (ploidy psi, purity rho) cell over S segments - the kernel, the host path of the same call, the
// entry point - and the sum rule alone for the tests.  Compiled with -ffp-contract=off: every sum, product and division below is the one
// numpy does, in its order.  DESIGN.md "ASCAT grid" derives the four rules.
//
// 1. The power depends on the segment only.  With s = (logR, BAF, probes) per segment the caller computes, with numpy itself,
//      u = (s[:,1] - 1) * 2 ** (s[:,0] / gamma),  w = s[:,1] * 2 ** (s[:,0] / gamma),  cnt = s[:,2],  wgt = where(s[:,1] == 0.5, 0.05, 1):
//    numpy's array power is not libm's pow on every build, and nothing here calls pow.
// 2. Per cell, with c = (1 - rho) * 2 + rho * psi:
//      nA = ((rho - 1) - u * c) / rho,  nB = ((rho - 1) + w * c) / rho,  sa = nansum(nA),  sb = nansum(nB),  m = sa < sb ? nA : nB,
//      t = m - max(rint(m), 0)  (rint rounds half to even; the max keeps a NaN),  d = nansum(((|t| * |t|) * cnt) * wgt).
// 3. nansum(a, n) = numpy's pairwise sum of a with every NaN replaced by 0.  pw(a, n) of one block:
//      n < 8: the values added in order into -0.0;
//      8 <= n <= 128: eight running sums r[j] = a[j] + a[8 + j] + ... over the first n - n % 8 values, combined as
//        ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the n % 8 values of the tail added in order;
//      n > 128: n2 = n / 2, n2 -= n2 % 8, pw(a, n2) + pw(a + n2, n - n2).
//    numpy reduces in buffers of 8192 values: the sum is ((0.0 + pw(first 8192)) + pw(next 8192)) + ...
//    The blocks of at most 128 values ("leaves") and the order in which their sums combine depend on n alone: the entry point lists
//    them once per call (leaf_table), and both paths follow that list.  A leaf's sum goes on a stack; `combines` says how many times
//    the two topmost entries are then replaced by their sum; `last` ends a buffer of 8192: the one entry left is added to the total.
// 4. The local-minimum scans that read d afterwards change it while they read it; they stay numpy on the host (run_ascat.py).
#include <algorithm>
#include <cmath>
#include <mutex>
#include <thread>
#include <vector>
#include "hip_buffers.h"

namespace {

using namespace cto;

constexpr int AC_THREADS = 256, AC_LANES = 8, AC_CELLS = AC_THREADS / AC_LANES;  // eight lanes per cell: a leaf's eight running sums
constexpr int AC_LEAF = 128, AC_BUFFER = 8192, AC_STACK = AC_LANES;               // the stack lives in the eight lanes
constexpr int AC_LDS_SEGMENTS = CTO_ASCAT_LDS_SEGMENTS;
static_assert(4 * 8 * AC_LDS_SEGMENTS <= 65536, "the four per-segment arrays must fit the LDS of one workgroup");

struct AcLeaf { int32_t start, len, combines, last; };

void add_leaves(int lo, int n, std::vector<AcLeaf>& out) {       // pw(a + lo, n)
    if (n <= AC_LEAF) {
        out.push_back(AcLeaf{lo, n, 0, 0});
        return;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    add_leaves(lo, n2, out);
    add_leaves(lo + n2, n - n2, out);
    out.back().combines += 1;
}

// the leaves of a sum over n values and the deepest the stack gets
std::vector<AcLeaf> leaf_table(int n, int* depth) {
    std::vector<AcLeaf> out;
    for (int lo = 0; lo < n; lo += AC_BUFFER) {
        add_leaves(lo, std::min(AC_BUFFER, n - lo), out);
        out.back().last = 1;
    }
    int sp = 0;
    *depth = 0;
    for (const AcLeaf& lf : out) {
        *depth = std::max(*depth, ++sp);
        sp -= lf.combines;
        if (lf.last) sp = 0;
    }
    return out;
}

inline double nan_to_zero(double v) { return v != v ? 0.0 : v; }

// ------------------------------------------------------------------------------------------------ host path
template <class F> double sum_by_table(const std::vector<AcLeaf>& leaves, F&& at) {       // at(i): the i-th value, NaN already 0
    double total = 0.0, stack[AC_STACK];
    int sp = 0;
    for (const AcLeaf& lf : leaves) {
        double res;
        if (lf.len < 8) {
            res = -0.0;
            for (int i = 0; i < lf.len; ++i) res += at(lf.start + i);
        } else {
            double r[8];
            for (int j = 0; j < 8; ++j) r[j] = at(lf.start + j);
            const int body = lf.len - lf.len % 8;
            for (int i = 8; i < body; i += 8)
                for (int j = 0; j < 8; ++j) r[j] += at(lf.start + i + j);
            res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
            for (int i = body; i < lf.len; ++i) res += at(lf.start + i);
        }
        stack[sp++] = res;
        for (int c = 0; c < lf.combines; ++c, --sp) stack[sp - 2] = stack[sp - 2] + stack[sp - 1];
        if (lf.last) {
            total += stack[0];
            sp = 0;
        }
    }
    return total;
}

inline double distance_term(double m, double cnt, double wgt) {
    const double r = std::rint(m), floor0 = r != r ? r : (r > 0.0 ? r : 0.0), t = std::fabs(m - floor0);
    return nan_to_zero(((t * t) * cnt) * wgt);
}

double cell_on_host(const std::vector<AcLeaf>& leaves, const double* u, const double* w, const double* cnt, const double* wgt, double psi, double rho) {
    const double rm1 = rho - 1.0, c = (1.0 - rho) * 2.0 + rho * psi;
    const double sa = sum_by_table(leaves, [&](int i) { return nan_to_zero((rm1 - u[i] * c) / rho); });
    const double sb = sum_by_table(leaves, [&](int i) { return nan_to_zero((rm1 + w[i] * c) / rho); });
    if (sa < sb) return sum_by_table(leaves, [&](int i) { return distance_term((rm1 - u[i] * c) / rho, cnt[i], wgt[i]); });
    return sum_by_table(leaves, [&](int i) { return distance_term((rm1 + w[i] * c) / rho, cnt[i], wgt[i]); });
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

// ------------------------------------------------------------------------------------------------ kernel
// K sums at once over the leaf table by the eight lanes [base, base + 8) of a wave (j = the lane's place among them).  term(i, v) fills
// v[0..K) with the i-th values, NaN already 0.  Lane j keeps the running sum r[j] of a leaf; three xor-shuffles give every lane the
// bracketed tree (a + b and b + a are the same bits); every lane adds the tail.  Stack entry k lives in lane k.  Every lane of the
// workgroup takes the same branches: the table is the same for all cells.
template <int K, class F>
__device__ inline void octet_nansum(const AcLeaf* __restrict__ leaves, int n_leaves, int j, int base, F&& term, double (&total)[K]) {
    double stack[K], r[K], v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) total[k] = stack[k] = 0.0;
    int sp = 0;
    for (int l = 0; l < n_leaves; ++l) {
        const AcLeaf lf = leaves[l];
        if (lf.len < 8) {
#pragma unroll
            for (int k = 0; k < K; ++k) r[k] = -0.0;
            for (int i = 0; i < lf.len; ++i) {
                term(lf.start + i, v);
#pragma unroll
                for (int k = 0; k < K; ++k) r[k] += v[k];
            }
        } else {
            const int body = lf.len - lf.len % 8;
            term(lf.start + j, r);
            for (int i = 8; i < body; i += 8) {
                term(lf.start + i + j, v);
#pragma unroll
                for (int k = 0; k < K; ++k) r[k] += v[k];
            }
#pragma unroll
            for (int o = 1; o < AC_LANES; o <<= 1) {
#pragma unroll
                for (int k = 0; k < K; ++k) r[k] += __shfl_xor(r[k], o);
            }
            for (int i = body; i < lf.len; ++i) {
                term(lf.start + i, v);
#pragma unroll
                for (int k = 0; k < K; ++k) r[k] += v[k];
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (j == sp) stack[k] = r[k];
        ++sp;
        for (int c = 0; c < lf.combines; ++c, --sp) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const double left = __shfl(stack[k], base + sp - 2), right = __shfl(stack[k], base + sp - 1);
                if (j == sp - 2) stack[k] = left + right;
            }
        }
        if (lf.last) {
#pragma unroll
            for (int k = 0; k < K; ++k) total[k] += __shfl(stack[k], base);
            sp = 0;
        }
    }
}

// AC_CELLS cells per workgroup, eight lanes each.  IN_LDS: the four per-segment arrays are copied to LDS first (S <= AC_LDS_SEGMENTS);
// otherwise they are read from global memory, where every cell reads the same addresses.  The lanes of a cell beyond the grid work on the
// last cell and store nothing.
template <bool IN_LDS>
__global__ __launch_bounds__(AC_THREADS) void k_ascat_distance(const double* __restrict__ g_u, const double* __restrict__ g_w,
                                                               const double* __restrict__ g_cnt, const double* __restrict__ g_wgt, int S,
                                                               const AcLeaf* __restrict__ leaves, int n_leaves, const double* __restrict__ psi,
                                                               const double* __restrict__ rho, int R, int n_cells, double* __restrict__ d) {
    extern __shared__ double s_in[];
    const int tid = threadIdx.x, j = tid & (AC_LANES - 1), base = (tid & 63) - j;
    const double *u = g_u, *w = g_w, *cnt = g_cnt, *wgt = g_wgt;
    if (IN_LDS) {
        for (int i = tid; i < S; i += AC_THREADS) {
            s_in[i] = g_u[i];
            s_in[S + i] = g_w[i];
            s_in[2 * S + i] = g_cnt[i];
            s_in[3 * S + i] = g_wgt[i];
        }
        __syncthreads();
        u = s_in;
        w = s_in + S;
        cnt = s_in + 2 * S;
        wgt = s_in + 3 * S;
    }
    const int cell_of_lane = blockIdx.x * AC_CELLS + tid / AC_LANES, cell = min(cell_of_lane, n_cells - 1);
    const double rh = rho[cell % R], ps = psi[cell / R];
    const double rm1 = rh - 1.0, c = (1.0 - rh) * 2.0 + rh * ps;

    double s[2];
    octet_nansum<2>(leaves, n_leaves, j, base, [&](int i, double (&v)[2]) {
        const double nA = (rm1 - u[i] * c) / rh, nB = (rm1 + w[i] * c) / rh;
        v[0] = nA != nA ? 0.0 : nA;
        v[1] = nB != nB ? 0.0 : nB;
    }, s);
    const bool minor_is_a = s[0] < s[1];
    double dist[1];
    octet_nansum<1>(leaves, n_leaves, j, base, [&](int i, double (&v)[1]) {
        const double m = (minor_is_a ? rm1 - u[i] * c : rm1 + w[i] * c) / rh;
        const double r = rint(m), floor0 = r != r ? r : (r > 0.0 ? r : 0.0), t = fabs(m - floor0);
        const double e = ((t * t) * cnt[i]) * wgt[i];
        v[0] = e != e ? 0.0 : e;
    }, dist);
    if (j == 0 && cell_of_lane < n_cells) d[cell] = dist[0];
}

struct AcContext : BatchCtx {};                                  // the device side, one call at a time: the buffers outlive the calls

}  // namespace

extern "C" int cto_ascat_distance(const double* u, const double* w, const double* cnt, const double* wgt, int64_t S, const double* psi, int64_t P,
                                  const double* rho, int64_t R, int where, double* d, cto_ascat_stats* stats) try {
    if (stats) *stats = cto_ascat_stats{0, 0, 0, 0.0};
    CTO_REQUIRE(S >= 1, CTO_EINVAL, "cto_ascat_distance: %lld segments", (long long)S);
    CTO_REQUIRE(P >= 1 && R >= 1, CTO_EINVAL, "cto_ascat_distance: a grid of %lld x %lld cells", (long long)P, (long long)R);
    CTO_REQUIRE(u && w && cnt && wgt && psi && rho && d, CTO_EINVAL, "cto_ascat_distance: null array");
    CTO_REQUIRE(where == 0 || where == 1, CTO_EINVAL, "cto_ascat_distance: where is %d, not 0 (device) or 1 (host)", where);
    CTO_REQUIRE(S <= CTO_ASCAT_MAX_SEGMENTS && P <= (1 << 20) && R <= (1 << 20) && P * R <= (1 << 28), CTO_EUNSUPPORTED,
                "cto_ascat_distance: %lld segments on a grid of %lld x %lld cells", (long long)S, (long long)P, (long long)R);
    for (int64_t jr = 0; jr < R; ++jr) CTO_REQUIRE(rho[jr] != 0.0, CTO_EINVAL, "cto_ascat_distance: purity %lld of the grid is 0", (long long)jr);
    const int64_t n_cells = P * R;
    int depth = 0;
    const std::vector<AcLeaf> leaves = leaf_table(int(S), &depth);
    CTO_REQUIRE(depth <= AC_STACK, CTO_EUNSUPPORTED, "cto_ascat_distance: a sum of %lld values stacks %d partial sums", (long long)S, depth);
    if (stats) { stats->n_cells = n_cells; stats->n_segments = S; }

    if (where == 1) {
        over_threads(size_t(n_cells), [&](size_t cell) { d[cell] = cell_on_host(leaves, u, w, cnt, wgt, psi[cell / size_t(R)], rho[cell % size_t(R)]); });
        if (stats) stats->host_path = 1;
        return CTO_OK;
    }
    int n_dev = 0;
    CTO_REQUIRE(hipGetDeviceCount(&n_dev) == hipSuccess && n_dev > 0, CTO_EHIP,
                "cto_ascat_distance: no HIP device (the host path is taken only when asked for)");

    // one upload: [u | w | cnt | wgt | psi | rho | leaves]; one download: d
    const size_t bytes_s = align16(size_t(S) * 8), bytes_p = align16(size_t(P) * 8), bytes_r = align16(size_t(R) * 8);
    const size_t off_w = bytes_s, off_cnt = 2 * bytes_s, off_wgt = 3 * bytes_s, off_psi = 4 * bytes_s, off_rho = off_psi + bytes_p,
                 off_leaves = off_rho + bytes_r, bytes_in = off_leaves + leaves.size() * sizeof(AcLeaf), bytes_out = size_t(n_cells) * 8;
    AcContext& X = process_wide<AcContext>();
    std::lock_guard<std::mutex> lock(X.mu);
    if (const int rc = X.open(bytes_in, bytes_out)) return rc;
    char* h = X.h_in.as<char>();
    memcpy(h, u, size_t(S) * 8);
    memcpy(h + off_w, w, size_t(S) * 8);
    memcpy(h + off_cnt, cnt, size_t(S) * 8);
    memcpy(h + off_wgt, wgt, size_t(S) * 8);
    memcpy(h + off_psi, psi, size_t(P) * 8);
    memcpy(h + off_rho, rho, size_t(R) * 8);
    memcpy(h + off_leaves, leaves.data(), leaves.size() * sizeof(AcLeaf));
    const char* dev = X.d_in.as<char>();
    CTO_HIP(hipMemcpyAsync(X.d_in.p, h, bytes_in, hipMemcpyHostToDevice, X.stream));
    CTO_HIP(hipEventRecord(X.ev0, X.stream));
    const bool in_lds = S <= AC_LDS_SEGMENTS;
    const dim3 grid(uint32_t((n_cells + AC_CELLS - 1) / AC_CELLS)), block(AC_THREADS);
    const auto kernel = in_lds ? k_ascat_distance<true> : k_ascat_distance<false>;
    hipLaunchKernelGGL(kernel, grid, block, in_lds ? size_t(S) * 32 : 0, X.stream, reinterpret_cast<const double*>(dev),
                       reinterpret_cast<const double*>(dev + off_w), reinterpret_cast<const double*>(dev + off_cnt),
                       reinterpret_cast<const double*>(dev + off_wgt), int(S), reinterpret_cast<const AcLeaf*>(dev + off_leaves), int(leaves.size()),
                       reinterpret_cast<const double*>(dev + off_psi), reinterpret_cast<const double*>(dev + off_rho), int(R), int(n_cells),
                       X.d_out.as<double>());
    CTO_HIP(hipGetLastError());
    CTO_HIP(hipEventRecord(X.ev1, X.stream));
    CTO_HIP(hipMemcpyAsync(X.h_out.p, X.d_out.p, bytes_out, hipMemcpyDeviceToHost, X.stream));
    CTO_HIP(record_and_wait(X.done, X.stream));
    if (stats) {
        float ms = 0.f;
        CTO_HIP(hipEventElapsedTime(&ms, X.ev0, X.ev1));
        stats->kernel_ms = ms;
    }
    memcpy(d, X.h_out.p, bytes_out);
    return CTO_OK;
}
CTO_CATCH("cto_ascat_distance", int)

// the sum rule alone, as both paths apply it (for the tests: numpy's order of additions is an observation, not a promise)
extern "C" int cto_ascat_sum(const double* x, int64_t n, double* out) try {
    CTO_REQUIRE(n >= 0 && (n == 0 || x) && out, CTO_EINVAL, "cto_ascat_sum: bad arguments");
    CTO_REQUIRE(n <= CTO_ASCAT_MAX_SEGMENTS, CTO_EUNSUPPORTED, "cto_ascat_sum: %lld values", (long long)n);
    int depth = 0;
    const std::vector<AcLeaf> leaves = leaf_table(int(n), &depth);
    CTO_REQUIRE(depth <= AC_STACK, CTO_EUNSUPPORTED, "cto_ascat_sum: a sum of %lld values stacks %d partial sums", (long long)n, depth);
    *out = sum_by_table(leaves, [&](int i) { return nan_to_zero(x[i]); });
    return CTO_OK;
}
CTO_CATCH("cto_ascat_sum", int)
