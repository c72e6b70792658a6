// correct_logr, step 3 of the Verdict chain (src/verdict/correct_logr.py of the reference): the tumour logR of N probes, regressed on
// cubic B-splines of two GC-content columns and one replication-timing column; the residuals are the corrected logR.  The kernels, the
// host path of the same call, the entry point - and the basis alone for the tests.  Compiled with -ffp-contract=off: both paths do the
// same operations in the same order and return the same bits.  DESIGN.md "logR correction" derives the rules.
//
// 1. Column choice.  For a table x (N x C, row-major) and the logR y, row 0 of np.corrcoef(x, y, rowvar=False) without its first entry:
//      corr[j - 1] = |clip(((S(0, j) * (1 / (N - 1))) / sd(0)) / sd(j))|,  j = 1 .. C,  column C being y,
//      S(0, j) = sum((x0 - mean(x0)) * (xj - mean(xj))),  sd(j) = sqrt(S(j, j) * (1 / (N - 1))),
//    two passes, as numpy does: the means first, then the sums of the centred values.  A constant column gives 0 / 0 = NaN.
//    insert = argmax(corr_gc[:6]), amplic = argmax(corr_gc[7:12]) + 7, replic = argmax(corr_rt); np.argmax takes the first NaN when
//    there is one.  The three results index the table's columns directly (one column off from what was correlated): kept.
// 2. Basis.  For a chosen column with minimum a and maximum b: the knots a a a a m b b b b, m = (b - a) / 2 + a; the four cubic
//    B-splines that are not zero at x by de Boor's recurrence, interval 3 for x < m and interval 4 otherwise (x == b included):
//      h = [1]; for j = 1, 2, 3: hh = h, h[0] = 0, and for n = 1 .. j with xb = t[ell + n], xa = t[ell + n - j]:
//        w = hh[n - 1] / (xb - xa),  h[n - 1] += w * (xb - x),  h[n] = w * (x - xa)       (h[n] = 0 where xb == xa)
//    - the bits of scipy's BSpline on every value tried, but for the two ends: x == a gives (1, 0, 0, 0, 0) and x == b gives
//    (0, 0, 0, 0, 1) exactly, where the recurrence's (1 / (m - a)) * (m - a) may round to 1 - 2^-53 (a deviation of at most three such
//    steps, in the rows that hold a column's extremes).  Five functions per column, each row of a block summing to 1.
// 3. Fit.  The reference's LinearRegression centres the 15 columns and y and asks for the minimum-norm solution of a design of rank
//    12; only the residuals are printed, and they are the projection of y off the column space, whatever the coefficients.  Here the
//    middle function of each block is dropped (the same space with the intercept, at full rank): 12 columns, centred by their means
//    (a pass of their own), the 13 x 13 sums of products of the centred columns and the centred y, a Cholesky solve of the 12 x 12
//    part on the host, the residuals r = yc - Xc beta, and one step of refinement: g = Xc' r and sum(r), a second solve, and
//    r -= sum(r) / N + Xc d.
// 4. Every sum over rows is one fixed tree, the same on both paths and for every launch: blocks of CL_ROWS rows, the partial sums of
//    the blocks combined pairwise (block i += block i + s for s = 1, 2, 4, ...).  Inside a block, the per-row kernels add the 256 rows
//    as a balanced binary tree (rows beyond N count as 0.0); the table kernels give row k of the block to slot k % R, R = the rows one
//    step of 256 threads covers with 16-byte loads = (512 / C) rounded down to even, add a slot's rows in order, and fold the slots
//    (slot i += slot i + h for h = P / 2 .. 1, P the power of two >= R).  No floating-point atomics.
// 5. Refused (CTO_EINVAL): N < 2, C_gc < 8, C_rt < 1, a value that is not finite (seen as a column sum that is not finite), a chosen
//    column with min == max (the reference dies there on NaN), a Cholesky pivot that is not positive, or below 64 ulp of its diagonal
//    entry (the reference's minimum-norm solve would still answer: a deviation; it takes a chosen column with no value in one half of
//    its range, or fewer rows than columns).
#include <algorithm>
#include <cmath>
#include <limits>
#include <mutex>
#include <vector>
#include "hip_buffers.h"

namespace {

using namespace cto;

#define CL_HD __host__ __device__ inline

constexpr int CL_ROWS = CTO_CORRECT_LOGR_BLOCK_ROWS, CL_THREADS = 256, CL_WAVES = CL_THREADS / 64;
constexpr int CL_MAX_COLS = CTO_CORRECT_LOGR_MAX_COLUMNS;
constexpr int CL_P = 12, CL_V = CL_P + 1, CL_GRAM = CL_V * (CL_V + 1) / 2, CL_COMBINE_THREADS = 1024;
static_assert(CL_ROWS == CL_THREADS && CL_ROWS % 2 == 0, "a per-row kernel's block is one row per thread; a table step starts on an even row");
constexpr int CL_SMALL = 2 * CL_MAX_COLS + 2;                    // the most values one phase returns or takes

struct ClFit { double lo[3], mid[3], hi[3], mean[CL_V]; };       // the knots of the three chosen columns; the means of the 12 columns and y
struct ClVec { double v[CL_V]; };                                // 12 coefficients, and the constant of the refinement step

// ------------------------------------------------------------------------------------------------ the arithmetic both paths share
CL_HD int step_rows(int C) { return (512 / C) & ~1; }

// rule 2: the five B-splines at x (the four of its interval, a zero for the fifth)
CL_HD void basis5(double x, double a, double m, double b, double (&B)[5]) {
    const bool low = x < m;
    const double t[7] = {a, a, a, low ? a : m, low ? m : b, b, b};             // the knots ell - 3 .. ell + 3
    double h[4] = {1.0, 0.0, 0.0, 0.0}, hh[4];
#pragma unroll
    for (int j = 1; j <= 3; ++j) {
#pragma unroll
        for (int i = 0; i < j; ++i) hh[i] = h[i];
        h[0] = 0.0;
#pragma unroll
        for (int n = 1; n <= j; ++n) {
            const double xb = t[3 + n], xa = t[3 + n - j];
            if (xb == xa) {
                h[n] = 0.0;
                continue;
            }
            const double w = hh[n - 1] / (xb - xa);
            h[n - 1] += w * (xb - x);
            h[n] = w * (x - xa);
        }
    }
    const bool first = x == a, last = x == b;                   // the ends are exact: w * (xb - xa) may round to 1 - 2^-53
    B[0] = first ? 1.0 : (low ? h[0] : 0.0);
    B[1] = first || last ? 0.0 : (low ? h[1] : h[0]);
    B[2] = first || last ? 0.0 : (low ? h[2] : h[1]);
    B[3] = first || last ? 0.0 : (low ? h[3] : h[2]);
    B[4] = last ? 1.0 : (low ? 0.0 : h[3]);
}

// rule 3: the 12 design values of a row, not centred
CL_HD void design_row(const double (&x)[3], const ClFit& f, double* v) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double B[5];
        basis5(x[k], f.lo[k], f.mid[k], f.hi[k], B);
        v[4 * k] = B[0];
        v[4 * k + 1] = B[1];
        v[4 * k + 2] = B[3];
        v[4 * k + 3] = B[4];
    }
}

CL_HD void centred_row(const double (&x)[3], double y, const ClFit& f, double (&v)[CL_V]) {
    design_row(x, f, v);
    v[CL_P] = y;
#pragma unroll
    for (int k = 0; k < CL_V; ++k) v[k] -= f.mean[k];
}

CL_HD void gram_row(const double (&v)[CL_V], double (&p)[CL_GRAM]) {           // the upper triangle, row by row
    int q = 0;
#pragma unroll
    for (int r = 0; r < CL_V; ++r) {
#pragma unroll
        for (int c = r; c < CL_V; ++c) p[q++] = v[r] * v[c];
    }
}

CL_HD double residual_of(const double (&v)[CL_V], const ClVec& beta) {
    double r = v[CL_P];
#pragma unroll
    for (int k = 0; k < CL_P; ++k) r -= v[k] * beta.v[k];
    return r;
}

CL_HD double corrected(double r, const double (&v)[CL_V], const ClVec& d) {
    r -= d.v[CL_P];
#pragma unroll
    for (int k = 0; k < CL_P; ++k) r -= v[k] * d.v[k];
    return r;
}

CL_HD double combine_op(int mode, int q, double a, double b) {                // mode 0: sums; mode 1: three minima, then three maxima
    if (mode == 0) return a + b;
    return q < 3 ? (b < a ? b : a) : (b > a ? b : a);
}

// ------------------------------------------------------------------------------------------------ host path
// rule 4, a table: acc[q * R + slot] over the rows of block b, then the fold of the slots -> out[0 .. Q)
template <int PASS>
void host_table_block(const double* x, int64_t N, int C, const double* logr, const double* mean, int64_t b, std::vector<double>& acc, double* out) {
    const int R = step_rows(C), Q = PASS == 1 ? C + 1 : 2 * C + 2;
    std::fill(acc.begin(), acc.begin() + size_t(Q) * R, 0.0);
    const int64_t rb = b * CL_ROWS, end = std::min<int64_t>(N, rb + CL_ROWS);
    for (int64_t row = rb; row < end; ++row) {
        const int s = int((row - rb) % R);
        const double* xr = x + row * C;
        if (PASS == 1) {
            for (int c = 0; c < C; ++c) acc[size_t(c) * R + s] += xr[c];
            acc[size_t(C) * R + s] += logr[row];
        } else {
            const double d0 = xr[0] - mean[0], l = logr[row] - mean[C];
            for (int c = 0; c < C; ++c) {
                const double d = xr[c] - mean[c];
                acc[size_t(c) * R + s] += d * d;
                acc[size_t(C + 1 + c) * R + s] += d * d0;
            }
            acc[size_t(C) * R + s] += l * l;
            acc[size_t(2 * C + 1) * R + s] += l * d0;
        }
    }
    int P = 1;
    while (P < R) P <<= 1;
    for (int q = 0; q < Q; ++q) {
        double* v = &acc[size_t(q) * R];
        for (int h = P / 2; h >= 1; h >>= 1)
            for (int i = 0; i < h; ++i)
                if (i + h < R) v[i] += v[i + h];
        out[q] = v[0];
    }
}

// rule 4, a per-row kernel's block: leaf[row in block * Q + q] -> out[0 .. Q), a balanced tree (mode as in combine_op)
void host_fold_rows(std::vector<double>& leaf, int Q, int mode, double* out) {
    for (int s = 1; s < CL_ROWS; s <<= 1)
        for (int i = 0; i < CL_ROWS; i += 2 * s)
            for (int q = 0; q < Q; ++q) leaf[size_t(i) * Q + q] = combine_op(mode, q, leaf[size_t(i) * Q + q], leaf[size_t(i + s) * Q + q]);
    std::copy(leaf.begin(), leaf.begin() + Q, out);
}

// rule 4, the blocks: part[b * Q + q] -> part[0 .. Q)
void host_combine(double* part, int64_t nb, int Q, int mode) {
    for (int64_t s = 1; s < nb; s <<= 1)
        for (int64_t i = 0; i + s < nb; i += 2 * s)
            for (int q = 0; q < Q; ++q) part[i * Q + q] = combine_op(mode, q, part[i * Q + q], part[(i + s) * Q + q]);
}

struct HostEngine {
    const double *logr, *gc, *rt;
    int64_t N, nb;
    int G, T;
    std::vector<double> xs, part, leaf;
    double* r;
    double kernel_ms = 0.0;

    template <int PASS> int table(int which, const double* mean, double* out) {
        const double* x = which ? rt : gc;
        const int C = which ? T : G, Q = PASS == 1 ? C + 1 : 2 * C + 2;
        std::vector<double> acc(size_t(Q) * step_rows(C));
        part.resize(size_t(nb) * Q);
        for (int64_t b = 0; b < nb; ++b) host_table_block<PASS>(x, N, C, logr, mean, b, acc, &part[size_t(b) * Q]);
        host_combine(part.data(), nb, Q, 0);
        std::copy(part.begin(), part.begin() + Q, out);
        return CTO_OK;
    }
    // leaf(row, v) fills the Q values of a row; rows beyond N hold `pad`
    template <class F> void per_row(int Q, int mode, double* out, F&& leaf_of) {
        part.resize(size_t(nb) * Q);
        leaf.resize(size_t(CL_ROWS) * Q);
        for (int64_t b = 0; b < nb; ++b) {
            for (int k = 0; k < CL_ROWS; ++k) {
                const int64_t row = b * CL_ROWS + k;
                double* v = &leaf[size_t(k) * Q];
                if (row < N) {
                    leaf_of(row, v);
                } else {
                    for (int q = 0; q < Q; ++q) v[q] = mode == 0 ? 0.0 : (q < 3 ? std::numeric_limits<double>::infinity() : -std::numeric_limits<double>::infinity());
                }
            }
            host_fold_rows(leaf, Q, mode, &part[size_t(b) * Q]);
        }
        host_combine(part.data(), nb, Q, mode);
        std::copy(part.begin(), part.begin() + Q, out);
    }
    void row_x(int64_t row, double (&x)[3]) const {
        for (int k = 0; k < 3; ++k) x[k] = xs[size_t(k) * N + row];
    }
    int gather(const int (&col)[3], double* out) {
        xs.resize(size_t(3) * N);
        per_row(6, 1, out, [&](int64_t row, double* v) {
            const double x[3] = {gc[row * G + col[0]], gc[row * G + col[1]], rt[row * T + col[2]]};
            for (int k = 0; k < 3; ++k) xs[size_t(k) * N + row] = v[k] = v[3 + k] = x[k];
        });
        return CTO_OK;
    }
    int basis_sums(const ClFit& f, double* out) {
        per_row(CL_P, 0, out, [&](int64_t row, double* v) {
            double x[3];
            row_x(row, x);
            design_row(x, f, v);
        });
        return CTO_OK;
    }
    int gram(const ClFit& f, double* out) {
        per_row(CL_GRAM, 0, out, [&](int64_t row, double* p) {
            double x[3], v[CL_V], g[CL_GRAM];
            row_x(row, x);
            centred_row(x, logr[row], f, v);
            gram_row(v, g);
            std::copy(g, g + CL_GRAM, p);
        });
        return CTO_OK;
    }
    int residuals(const ClFit& f, const ClVec& beta, double* out) {
        per_row(CL_V, 0, out, [&](int64_t row, double* w) {
            double x[3], v[CL_V];
            row_x(row, x);
            centred_row(x, logr[row], f, v);
            const double res = residual_of(v, beta);
            r[row] = res;
            for (int k = 0; k < CL_P; ++k) w[k] = v[k] * res;
            w[CL_P] = res;
        });
        return CTO_OK;
    }
    int correct(const ClFit& f, const ClVec& d) {
        for (int64_t row = 0; row < N; ++row) {
            double x[3], v[CL_V];
            row_x(row, x);
            centred_row(x, logr[row], f, v);
            r[row] = corrected(r[row], v, d);
        }
        return CTO_OK;
    }
};

// ------------------------------------------------------------------------------------------------ kernels
// the Q values of every thread of the block -> part[0 .. Q): a butterfly inside each wave (lane 0 ends with the balanced tree over its
// 64 rows, itself the left operand at every level), then (wave 0 + wave 1) + (wave 2 + wave 3)
template <int Q> __device__ inline void block_fold(const double (&v)[Q], int mode, double* __restrict__ part) {
    __shared__ double s_wave[CL_WAVES * Q];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        double s = v[q];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const double other = __shfl_xor(s, o);
            s = (lane & o) ? combine_op(mode, q, other, s) : combine_op(mode, q, s, other);
        }
        if (lane == 0) s_wave[wave * Q + q] = s;
    }
    __syncthreads();
    for (int q = tid; q < Q; q += CL_THREADS)
        part[q] = combine_op(mode, q, combine_op(mode, q, s_wave[q], s_wave[Q + q]), combine_op(mode, q, s_wave[2 * Q + q], s_wave[3 * Q + q]));
}

// Phase (a).  One step covers R = step_rows(C) rows, R * C contiguous values: thread u loads values 2u and 2u + 1 of the step as 16
// bytes (the step starts on an even row, so on 16 bytes), which lie in the same slot and column at every step.  PASS 1: the column sums
// and the sum of logR; PASS 2: of the values centred by `mean` (C columns, then logR), the squares and the products with column 0.
template <int PASS>
__global__ __launch_bounds__(CL_THREADS) void k_table(const double* __restrict__ x, int64_t N, int C, const double* __restrict__ logr,
                                                      const double* __restrict__ mean, double* __restrict__ part) {
    extern __shared__ double s_acc[];                            // [Q][R + 1]
    const int R = step_rows(C), Q = PASS == 1 ? C + 1 : 2 * C + 2, W = R + 1, tid = threadIdx.x;
    const bool active = tid < R * C / 2;
    const int e0 = 2 * tid, slot[2] = {e0 / C, (e0 + 1) / C}, col[2] = {e0 % C, (e0 + 1) % C};
    const int64_t rb = int64_t(blockIdx.x) * CL_ROWS, end = rb + CL_ROWS < N ? rb + CL_ROWS : N;
    double a[2] = {0.0, 0.0}, p[2] = {0.0, 0.0}, al[2] = {0.0, 0.0}, pl[2] = {0.0, 0.0};     // al, pl: the logR, added by who holds column 0
    double m[2] = {0.0, 0.0}, mx = 0.0, ml = 0.0;
    if (PASS == 2 && active) {
        m[0] = mean[col[0]];
        m[1] = mean[col[1]];
        mx = mean[0];
        ml = mean[C];
    }
    if (active) {
        for (int at = 0; at < CL_ROWS; at += R) {
            const int64_t r0 = rb + at, row[2] = {r0 + slot[0], r0 + slot[1]};
            if (row[0] >= end) break;
            const double* src = x + r0 * C + e0;
            const int n = row[1] < end ? 2 : 1;
            double v[2] = {0.0, 0.0};
            if (n == 2) {
                const double2 both = *reinterpret_cast<const double2*>(src);
                v[0] = both.x;
                v[1] = both.y;
            } else {
                v[0] = *src;
            }
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (k >= n) break;
                if (PASS == 1) {
                    a[k] += v[k];
                    if (col[k] == 0) al[k] += logr[row[k]];
                } else {
                    const double d = v[k] - m[k], x0 = x[row[k] * C] - mx;
                    a[k] += d * d;
                    p[k] += d * x0;
                    if (col[k] == 0) {
                        const double l = logr[row[k]] - ml;
                        al[k] += l * l;
                        pl[k] += l * x0;
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            s_acc[col[k] * W + slot[k]] = a[k];
            if (col[k] == 0) s_acc[C * W + slot[k]] = al[k];
            if (PASS == 2) {
                s_acc[(C + 1 + col[k]) * W + slot[k]] = p[k];
                if (col[k] == 0) s_acc[(2 * C + 1) * W + slot[k]] = pl[k];
            }
        }
    }
    __syncthreads();
    int P = 1;
    while (P < R) P <<= 1;
    for (int q = tid; q < Q; q += CL_THREADS) {
        double* v = s_acc + q * W;
        for (int h = P / 2; h >= 1; h >>= 1)
            for (int i = 0; i < h; ++i)
                if (i + h < R) v[i] += v[i + h];
        part[int64_t(blockIdx.x) * Q + q] = v[0];
    }
}

// rule 4, the blocks: one workgroup folds part[b * Q + q] into part[0 .. Q)
__global__ __launch_bounds__(CL_COMBINE_THREADS) void k_combine(double* __restrict__ part, int64_t nb, int Q, int mode) {
    for (int64_t s = 1; s < nb; s <<= 1) {
        const int64_t pairs = (nb - s + 2 * s - 1) / (2 * s);    // the blocks i = 0, 2s, 4s, ... with i + s < nb
        for (int64_t k = threadIdx.x; k < pairs * Q; k += CL_COMBINE_THREADS) {
            const int64_t i = (k / Q) * 2 * s;
            const int q = int(k % Q);
            part[i * Q + q] = combine_op(mode, q, part[i * Q + q], part[(i + s) * Q + q]);
        }
        __syncthreads();
    }
}

// Phase (b): the three chosen columns, copied next to each other (xs[k * N + row]), and their ranges
__global__ __launch_bounds__(CL_THREADS) void k_gather(const double* __restrict__ gc, int G, const double* __restrict__ rt, int T, int col0, int col1,
                                                       int col2, int64_t N, double* __restrict__ xs, double* __restrict__ part) {
    const int64_t row = int64_t(blockIdx.x) * CL_ROWS + threadIdx.x;
    const double inf = __builtin_huge_val();
    double v[6] = {inf, inf, inf, -inf, -inf, -inf};
    if (row < N) {
        const double x[3] = {gc[row * G + col0], gc[row * G + col1], rt[row * T + col2]};
#pragma unroll
        for (int k = 0; k < 3; ++k) xs[k * N + row] = v[k] = v[3 + k] = x[k];
    }
    block_fold<6>(v, 1, part + int64_t(blockIdx.x) * 6);
}

__device__ inline bool load_row(const double* __restrict__ xs, int64_t N, double (&x)[3]) {
    const int64_t row = int64_t(blockIdx.x) * CL_ROWS + threadIdx.x;
    if (row >= N) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = xs[k * N + row];
    return true;
}

// Phase (c), first pass: the sums of the 12 design columns
__global__ __launch_bounds__(CL_THREADS) void k_basis_sums(const double* __restrict__ xs, int64_t N, ClFit f, double* __restrict__ part) {
    double x[3], v[CL_P];
#pragma unroll
    for (int k = 0; k < CL_P; ++k) v[k] = 0.0;
    if (load_row(xs, N, x)) design_row(x, f, v);
    block_fold<CL_P>(v, 0, part + int64_t(blockIdx.x) * CL_P);
}

// Phase (c), second pass: the 91 sums of products of the centred columns and the centred y
__global__ __launch_bounds__(CL_THREADS) void k_gram(const double* __restrict__ xs, const double* __restrict__ logr, int64_t N, ClFit f,
                                                     double* __restrict__ part) {
    double x[3], v[CL_V], p[CL_GRAM];
    if (load_row(xs, N, x)) {
        centred_row(x, logr[int64_t(blockIdx.x) * CL_ROWS + threadIdx.x], f, v);
        gram_row(v, p);
    } else {
#pragma unroll
        for (int q = 0; q < CL_GRAM; ++q) p[q] = 0.0;
    }
    block_fold<CL_GRAM>(p, 0, part + int64_t(blockIdx.x) * CL_GRAM);
}

// Phase (e): the residuals, and for the refinement step the sums of every centred column times the residual and of the residual
__global__ __launch_bounds__(CL_THREADS) void k_residuals(const double* __restrict__ xs, const double* __restrict__ logr, int64_t N, ClFit f, ClVec beta,
                                                          double* __restrict__ r, double* __restrict__ part) {
    double x[3], v[CL_V], w[CL_V];
#pragma unroll
    for (int k = 0; k < CL_V; ++k) w[k] = 0.0;
    if (load_row(xs, N, x)) {
        const int64_t row = int64_t(blockIdx.x) * CL_ROWS + threadIdx.x;
        centred_row(x, logr[row], f, v);
        const double res = residual_of(v, beta);
        r[row] = res;
#pragma unroll
        for (int k = 0; k < CL_P; ++k) w[k] = v[k] * res;
        w[CL_P] = res;
    }
    block_fold<CL_V>(w, 0, part + int64_t(blockIdx.x) * CL_V);
}

__global__ __launch_bounds__(CL_THREADS) void k_correct(const double* __restrict__ xs, const double* __restrict__ logr, int64_t N, ClFit f, ClVec d,
                                                        double* __restrict__ r) {
    double x[3], v[CL_V];
    if (load_row(xs, N, x)) {
        const int64_t row = int64_t(blockIdx.x) * CL_ROWS + threadIdx.x;
        centred_row(x, logr[row], f, v);
        r[row] = corrected(r[row], v, d);
    }
}

// the device side, one call at a time: the buffers outlive the calls.  h_in / d_in carry the few values a phase takes (the means),
// h_out the few it returns and then the residuals.
struct ClContext : BatchCtx {
    DevBuf data, work;                                           // [logr | gc | rt]; [xs | part]
};

struct DeviceEngine {
    ClContext& X;
    int64_t N, nb;
    int G, T;
    const double *logr = nullptr, *gc = nullptr, *rt = nullptr;
    double *xs = nullptr, *part = nullptr, *r = nullptr;
    double kernel_ms = 0.0;

    int open(const double* h_logr, const double* h_gc, const double* h_rt) {
        const size_t b_logr = align16(size_t(N) * 8), b_gc = align16(size_t(N) * G * 8), b_rt = align16(size_t(N) * T * 8);
        const size_t q_max = size_t(std::max(2 * std::max(G, T) + 2, CL_GRAM));
        int rc;
        if ((rc = X.open(CL_SMALL * 8, std::max(size_t(N), size_t(CL_SMALL)) * 8))) return rc;
        if ((rc = X.data.ensure(b_logr + b_gc + b_rt)) || (rc = X.work.ensure(align16(size_t(3) * N * 8) + size_t(nb) * q_max * 8))) return rc;
        char* d = X.data.as<char>();
        CTO_HIP(hipMemcpyAsync(d, h_logr, size_t(N) * 8, hipMemcpyHostToDevice, X.stream));
        CTO_HIP(hipMemcpyAsync(d + b_logr, h_gc, size_t(N) * G * 8, hipMemcpyHostToDevice, X.stream));
        CTO_HIP(hipMemcpyAsync(d + b_logr + b_gc, h_rt, size_t(N) * T * 8, hipMemcpyHostToDevice, X.stream));
        logr = reinterpret_cast<const double*>(d);
        gc = reinterpret_cast<const double*>(d + b_logr);
        rt = reinterpret_cast<const double*>(d + b_logr + b_gc);
        xs = X.work.as<double>();
        part = reinterpret_cast<double*>(X.work.as<char>() + align16(size_t(3) * N * 8));
        r = X.d_out.as<double>();
        return CTO_OK;
    }
    // the kernels of a phase are queued between begin() and end(); end() folds the blocks, waits and hands out part[0 .. Q)
    int begin() {
        CTO_HIP(hipEventRecord(X.ev0, X.stream));
        return CTO_OK;
    }
    int end(int Q, int mode, double* out) {
        CTO_HIP(hipGetLastError());
        if (Q) {
            hipLaunchKernelGGL(k_combine, dim3(1), dim3(CL_COMBINE_THREADS), 0, X.stream, part, nb, Q, mode);
            CTO_HIP(hipGetLastError());
        }
        CTO_HIP(hipEventRecord(X.ev1, X.stream));
        if (Q) CTO_HIP(hipMemcpyAsync(X.h_out.p, part, size_t(Q) * 8, hipMemcpyDeviceToHost, X.stream));
        CTO_HIP(record_and_wait(X.done, X.stream));
        float ms = 0.f;
        CTO_HIP(hipEventElapsedTime(&ms, X.ev0, X.ev1));
        kernel_ms += ms;
        if (Q) memcpy(out, X.h_out.p, size_t(Q) * 8);
        return CTO_OK;
    }
    template <int PASS> int table(int which, const double* mean, double* out) {
        const double* x = which ? rt : gc;
        const int C = which ? T : G, Q = PASS == 1 ? C + 1 : 2 * C + 2;
        if (PASS == 2) {
            memcpy(X.h_in.p, mean, size_t(C + 1) * 8);
            CTO_HIP(hipMemcpyAsync(X.d_in.p, X.h_in.p, size_t(C + 1) * 8, hipMemcpyHostToDevice, X.stream));
        }
        if (const int rc = begin()) return rc;
        hipLaunchKernelGGL(k_table<PASS>, dim3(uint32_t(nb)), dim3(CL_THREADS), size_t(Q) * (step_rows(C) + 1) * 8, X.stream, x, N, C, logr,
                           X.d_in.as<double>(), part);
        return end(Q, 0, out);
    }
    int gather(const int (&col)[3], double* out) {
        if (const int rc = begin()) return rc;
        hipLaunchKernelGGL(k_gather, dim3(uint32_t(nb)), dim3(CL_THREADS), 0, X.stream, gc, G, rt, T, col[0], col[1], col[2], N, xs, part);
        return end(6, 1, out);
    }
    int basis_sums(const ClFit& f, double* out) {
        if (const int rc = begin()) return rc;
        hipLaunchKernelGGL(k_basis_sums, dim3(uint32_t(nb)), dim3(CL_THREADS), 0, X.stream, xs, N, f, part);
        return end(CL_P, 0, out);
    }
    int gram(const ClFit& f, double* out) {
        if (const int rc = begin()) return rc;
        hipLaunchKernelGGL(k_gram, dim3(uint32_t(nb)), dim3(CL_THREADS), 0, X.stream, xs, logr, N, f, part);
        return end(CL_GRAM, 0, out);
    }
    int residuals(const ClFit& f, const ClVec& beta, double* out) {
        if (const int rc = begin()) return rc;
        hipLaunchKernelGGL(k_residuals, dim3(uint32_t(nb)), dim3(CL_THREADS), 0, X.stream, xs, logr, N, f, beta, r, part);
        return end(CL_V, 0, out);
    }
    int correct(const ClFit& f, const ClVec& d) {
        if (const int rc = begin()) return rc;
        hipLaunchKernelGGL(k_correct, dim3(uint32_t(nb)), dim3(CL_THREADS), 0, X.stream, xs, logr, N, f, d, r);
        return end(0, 0, nullptr);
    }
    int download(double* residual) {
        CTO_HIP(hipMemcpyAsync(X.h_out.p, r, size_t(N) * 8, hipMemcpyDeviceToHost, X.stream));
        CTO_HIP(record_and_wait(X.done, X.stream));
        memcpy(residual, X.h_out.p, size_t(N) * 8);
        return CTO_OK;
    }
};

// ------------------------------------------------------------------------------------------------ the steps between the phases (host)
bool all_finite(const double* v, int n) {
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

// rule 1: corr[0 .. C) from the sums of the second pass (squares [0 .. C], products with column 0 [C + 1 .. 2C + 1])
void correlations(const double* s2, int C, int64_t N, double* corr) {
    const double inv = 1.0 / double(N - 1), sd0 = std::sqrt(s2[0] * inv);
    for (int j = 1; j <= C; ++j) {
        double v = ((s2[C + 1 + j] * inv) / sd0) / std::sqrt(s2[j] * inv);
        v = v > 1.0 ? 1.0 : (v < -1.0 ? -1.0 : v);
        corr[j - 1] = std::fabs(v);
    }
}

int argmax_first_nan(const double* v, int lo, int hi) {          // np.argmax(v[lo:hi]) + lo, Python's slice rules
    int best = lo;
    for (int i = lo; i < hi; ++i) {
        if (v[i] != v[i]) return i;
        if (v[i] > v[best]) best = i;
    }
    return best;
}

// the solve G z = b by Cholesky, G = the 12 x 12 part of the packed upper triangle `gram`; false at a pivot that is not positive (one
// below 64 ulp of its diagonal entry is rounding noise: a column that the ones before it span)
bool cholesky(const double* gram, double (&L)[CL_P][CL_P], double (&b)[CL_P], int* bad) {
    double A[CL_V][CL_V];
    for (int r = 0, q = 0; r < CL_V; ++r)
        for (int c = r; c < CL_V; ++c, ++q) A[r][c] = A[c][r] = gram[q];
    for (int j = 0; j < CL_P; ++j) b[j] = A[j][CL_P];            // the right-hand side: every column times y
    for (int j = 0; j < CL_P; ++j) {
        double d = A[j][j];
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
        if (!(d > 64.0 * std::numeric_limits<double>::epsilon() * A[j][j]) || !std::isfinite(d)) {       // not positive beyond the rounding of the j terms
            *bad = j;
            return false;
        }
        L[j][j] = std::sqrt(d);
        for (int i = j + 1; i < CL_P; ++i) {
            double s = A[i][j];
            for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
            L[i][j] = s / L[j][j];
        }
    }
    return true;
}

void solve(const double (&L)[CL_P][CL_P], const double* b, double* z) {
    double y[CL_P];
    for (int i = 0; i < CL_P; ++i) {
        double s = b[i];
        for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
        y[i] = s / L[i][i];
    }
    for (int i = CL_P - 1; i >= 0; --i) {
        double s = y[i];
        for (int k = i + 1; k < CL_P; ++k) s -= L[k][i] * z[k];
        z[i] = s / L[i][i];
    }
}

template <class E>
int correct_logr(E& e, int64_t N, int G, int T, double* corr_gc, double* corr_rt, cto_correct_logr_stats* stats) {
    int rc;
    double out[CL_SMALL], mean[CL_MAX_COLS + 1];
    double y_mean = 0.0;
    for (int which = 0; which < 2; ++which) {                    // (a)
        const int C = which ? T : G;
        if ((rc = e.template table<1>(which, nullptr, out))) return rc;
        CTO_REQUIRE(all_finite(out, C + 1), CTO_EINVAL, "cto_correct_logr: a value that is not finite in the logR or the %s table (a column sum is not finite)",
                    which ? "replication-timing" : "GC");
        for (int c = 0; c <= C; ++c) mean[c] = out[c] / double(N);
        if (which == 0) y_mean = mean[C];
        if ((rc = e.template table<2>(which, mean, out))) return rc;
        correlations(out, C, N, which ? corr_rt : corr_gc);
    }
    const int col[3] = {argmax_first_nan(corr_gc, 0, std::min(6, G)), argmax_first_nan(corr_gc, 7, std::min(12, G)), argmax_first_nan(corr_rt, 0, T)};
    if (stats) {
        stats->col_insert = col[0];
        stats->col_amplic = col[1];
        stats->col_replic = col[2];
    }
    ClFit f;
    if ((rc = e.gather(col, out))) return rc;                    // (b)
    for (int k = 0; k < 3; ++k) {
        CTO_REQUIRE(out[k] < out[3 + k], CTO_EINVAL, "cto_correct_logr: column %d of the %s table, chosen for the fit, is constant (%.17g)", col[k],
                    k < 2 ? "GC" : "replication-timing", out[k]);
        f.lo[k] = out[k];
        f.hi[k] = out[3 + k];
        f.mid[k] = (f.hi[k] - f.lo[k]) / 2.0 + f.lo[k];
    }
    if ((rc = e.basis_sums(f, out))) return rc;                  // (c)
    for (int k = 0; k < CL_P; ++k) f.mean[k] = out[k] / double(N);
    f.mean[CL_P] = y_mean;
    if ((rc = e.gram(f, out))) return rc;
    double L[CL_P][CL_P] = {}, b[CL_P];                          // (d)
    int bad = 0;
    CTO_REQUIRE(cholesky(out, L, b, &bad), CTO_EINVAL,
                "cto_correct_logr: pivot %d of the Cholesky factor is not positive: %s column %d gives its functions no full rank (no value in one "
                "half of its range, or too few rows)", bad,
                bad < 8 ? "GC" : "replication-timing", col[bad / 4]);
    ClVec beta, d;
    solve(L, b, beta.v);
    beta.v[CL_P] = 0.0;
    if ((rc = e.residuals(f, beta, out))) return rc;             // (e)
    solve(L, out, d.v);
    d.v[CL_P] = out[CL_P] / double(N);
    return e.correct(f, d);
}

}  // namespace

extern "C" int cto_correct_logr(const double* logr, int64_t N, const double* gc, int64_t G, const double* rt, int64_t T, int where, double* corr_gc,
                                double* corr_rt, double* residual, cto_correct_logr_stats* stats) try {
    if (stats) *stats = cto_correct_logr_stats{0, 0, 0, -1, -1, -1, 0, 0.0};
    CTO_REQUIRE(N >= 2, CTO_EINVAL, "cto_correct_logr: %lld rows, fewer than 2", (long long)N);
    CTO_REQUIRE(G >= 8 && T >= 1, CTO_EINVAL, "cto_correct_logr: %lld GC columns (at least 8: the second window starts at entry 7) and %lld replication-timing columns (at least 1)",
                (long long)G, (long long)T);
    CTO_REQUIRE(logr && gc && rt && corr_gc && corr_rt && residual, CTO_EINVAL, "cto_correct_logr: null array");
    CTO_REQUIRE(where == 0 || where == 1, CTO_EINVAL, "cto_correct_logr: where is %d, not 0 (device) or 1 (host)", where);
    CTO_REQUIRE(N <= CTO_CORRECT_LOGR_MAX_ROWS && G <= CL_MAX_COLS && T <= CL_MAX_COLS, CTO_EUNSUPPORTED,
                "cto_correct_logr: %lld rows with %lld and %lld columns", (long long)N, (long long)G, (long long)T);
    if (stats) { stats->n_rows = N; stats->n_gc = G; stats->n_rt = T; }
    const int64_t nb = cdiv(N, CL_ROWS);
    if (where == 1) {
        HostEngine e{logr, gc, rt, N, nb, int(G), int(T), {}, {}, {}, residual};
        if (stats) stats->host_path = 1;
        return correct_logr(e, N, int(G), int(T), corr_gc, corr_rt, stats);
    }
    int n_dev = 0;
    CTO_REQUIRE(hipGetDeviceCount(&n_dev) == hipSuccess && n_dev > 0, CTO_EHIP,
                "cto_correct_logr: no HIP device (the host path is taken only when asked for)");
    ClContext& X = process_wide<ClContext>();
    std::lock_guard<std::mutex> lock(X.mu);
    DeviceEngine e{X, N, nb, int(G), int(T)};
    if (const int rc = e.open(logr, gc, rt)) return rc;
    const int rc = correct_logr(e, N, int(G), int(T), corr_gc, corr_rt, stats);
    if (stats) stats->kernel_ms = e.kernel_ms;
    if (rc) {
        (void)hipStreamSynchronize(X.stream);                    // nothing of this call is left queued on the buffers
        return rc;
    }
    return e.download(residual);
}
CTO_CATCH("cto_correct_logr", int)

// rule 2 alone, as both paths apply it (for the tests): the five B-splines of every x on the knots of [lo, hi], n x 5 row-major
extern "C" int cto_correct_logr_basis(const double* x, int64_t n, double lo, double hi, double* out) try {
    CTO_REQUIRE(n >= 0 && (n == 0 || (x && out)), CTO_EINVAL, "cto_correct_logr_basis: bad arguments");
    CTO_REQUIRE(lo < hi, CTO_EINVAL, "cto_correct_logr_basis: the range %.17g .. %.17g is empty", lo, hi);
    const double mid = (hi - lo) / 2.0 + lo;
    for (int64_t i = 0; i < n; ++i) {
        double B[5];
        basis5(x[i], lo, mid, hi, B);
        std::copy(B, B + 5, out + 5 * i);
    }
    return CTO_OK;
}
CTO_CATCH("cto_correct_logr_basis", int)
