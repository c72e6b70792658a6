// Exclusive prefix sums of int arrays on the device: one workgroup for short arrays, tile sums / their scan / every tile on top of its
// base for long ones.  Included by pileup.hip, extract.hip, allelecount.hip, aftally.hip, hapwindows.hip, phase.hip, contam.hip, pon.hip,
// addback.hip and comparevcf.hip, directly or through bam_records.h, lines.h and sort.h, and by primitives.hip, whose entries the tests
// call (tests/test_gpu_primitives.py).  In an anonymous namespace: every translation unit that includes it has its own kernels.
#pragma once
#include "common.h"

namespace {

// Exclusive prefix sum across the 1024 threads of the one workgroup these scan kernels run as (wave shuffles, then the 16 wave
// totals through LDS); *total = the sum.  Two barriers.
__device__ __forceinline__ long long block_scan_excl(long long v, long long* total, long long* wsum /* [17] shared */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long u = __shfl_up(inc, d);
        if (lane >= d) inc += u;
    }
    __syncthreads();                                          // wsum may still be read from the previous call
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    long long before = 0, all = 0;
    for (int w = 0; w < 16; ++w) { const long long x = wsum[w]; if (w < wave) before += x; all += x; }
    *total = all;
    return before + inc - v;
}

// exclusive prefix sums of an int array by one workgroup of 1024 threads, 4096 elements per pass (coalesced).  `in` and `out` may be
// the same array: a thread reads its four elements of a pass before the pass's barriers and writes back only those.
template <typename Out>
__global__ __launch_bounds__(1024) void k_scan_small(const int* in, Out* out, int n, Out* total) {
    __shared__ long long wsum[17];
    const int t = threadIdx.x;
    long long carry = 0;
    for (int base = 0; base < n; base += 4096) {
        const int i0 = base + 4 * t;
        int v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = i0 + k < n ? in[i0 + k] : 0;
        long long tot;
        long long ex = carry + block_scan_excl((long long)v[0] + v[1] + v[2] + v[3], &tot, wsum);
#pragma unroll
        for (int k = 0; k < 4; ++k) { if (i0 + k < n) out[i0 + k] = Out(ex); ex += v[k]; }
        carry += tot;
    }
    if (t == 0) { out[n] = Out(carry); if (total) *total = Out(carry); }
}

// The same over arrays of any length, spread over the chip: block sums of 4096-element tiles, their scan by one workgroup, then
// every tile scans itself on top of its base (a region piled up at every position has a million columns: the one-workgroup
// form above took 0.7 ms for them, the three launches below ~15 us).
constexpr int SCAN_TILE = 4096;
__global__ __launch_bounds__(1024) void k_tile_sums(const int* __restrict__ in, int n, long long* __restrict__ tsum) {
    __shared__ long long wsum[17];
    const int i0 = blockIdx.x * SCAN_TILE + 4 * threadIdx.x;
    long long v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) v += i0 + k < n ? in[i0 + k] : 0;
    long long tot;
    (void)block_scan_excl(v, &tot, wsum);
    if (threadIdx.x == 0) tsum[blockIdx.x] = tot;
}
// exclusive scan in place of up to three interleaved arrays of tile sums (a[i * stride + j], j < stride) by one workgroup;
// totals[j] receives the sums
__global__ __launch_bounds__(1024) void k_scan_tiles(long long* __restrict__ a, int n, int stride, long long* __restrict__ totals) {
    __shared__ long long wsum[17];
    const int t = threadIdx.x;
    for (int j = 0; j < stride; ++j) {
        long long carry = 0;
        for (int base = 0; base < n; base += 1024) {
            const int i = base + t;
            const long long v = i < n ? a[size_t(i) * stride + j] : 0;
            long long tot;
            const long long ex = carry + block_scan_excl(v, &tot, wsum);
            if (i < n) a[size_t(i) * stride + j] = ex;
            carry += tot;
        }
        if (t == 0) totals[j] = carry;
        __syncthreads();
    }
}
template <typename Out>
__global__ __launch_bounds__(1024) void k_scan_apply(const int* __restrict__ in, Out* __restrict__ out, int n, const long long* __restrict__ tbase,
                                                     const long long* __restrict__ totals, Out* total) {
    __shared__ long long wsum[17];
    const int i0 = blockIdx.x * SCAN_TILE + 4 * threadIdx.x;
    int v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = i0 + k < n ? in[i0 + k] : 0;
    long long tot;
    long long ex = tbase[blockIdx.x] + block_scan_excl((long long)v[0] + v[1] + v[2] + v[3], &tot, wsum);
#pragma unroll
    for (int k = 0; k < 4; ++k) { if (i0 + k < n) out[i0 + k] = Out(ex); ex += v[k]; }
    if (blockIdx.x == 0 && threadIdx.x == 0) { out[n] = Out(totals[0]); if (total) *total = Out(totals[0]); }
}

// out[0, n] = the exclusive prefix sums of in[0, n), out[n] (and *total, when given) their sum, on stream `s`.  Up to four tiles
// one workgroup does it in one launch; longer arrays take the three spread launches, with tile_tmp [cdiv(n, SCAN_TILE)] and
// tile_tot [1] as their scratch.  Launch errors are the caller's to collect (hipGetLastError).
template <typename Out>
void scan_exclusive(hipStream_t s, const int* in, int n, Out* out, Out* total, long long* tile_tmp, long long* tile_tot) {
    if (n <= 4 * SCAN_TILE) {
        hipLaunchKernelGGL(k_scan_small<Out>, dim3(1), dim3(1024), 0, s, in, out, n, total);
        return;
    }
    const int tiles = int(cto::cdiv(n, SCAN_TILE));
    hipLaunchKernelGGL(k_tile_sums, dim3(unsigned(tiles)), dim3(1024), 0, s, in, n, tile_tmp);
    hipLaunchKernelGGL(k_scan_tiles, dim3(1), dim3(1024), 0, s, tile_tmp, tiles, 1, tile_tot);
    hipLaunchKernelGGL(k_scan_apply<Out>, dim3(unsigned(tiles)), dim3(1024), 0, s, in, out, n, tile_tmp, tile_tot, total);
}

}  // namespace
