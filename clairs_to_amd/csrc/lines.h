// Line starts of a text on the device, in file order (pon.hip, addback.hip): k_line_count / scan_exclusive / k_line_emit, 16 KiB of
// text per workgroup.  In an anonymous namespace: every translation unit that includes it has its own kernels.
#pragma once
#include "scan.h"

namespace {

constexpr int LINE_TILE = 16384;                       // bytes of text per workgroup of the line-start passes: 16 per thread

__device__ __forceinline__ bool ends_line(uint8_t prev, uint8_t cur, int cr) { return prev == '\n' || (cr && prev == '\r' && cur != '\n'); }

// 16 bytes of text at `i0` (a multiple of 16) and the byte before them; zeros behind n
__device__ __forceinline__ void load16(const uint8_t* __restrict__ text, uint32_t n, uint32_t i0, uint8_t (&b)[16], uint8_t* prev) {
    if (i0 + 16 <= n) {
        const uint4 v = *reinterpret_cast<const uint4*>(text + i0);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 16; ++k) b[k] = uint8_t(w[k >> 2] >> (8 * (k & 3)));
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k) b[k] = i0 + k < n ? text[i0 + k] : 0;
    }
    *prev = i0 > 0 && i0 - 1 < n ? text[i0 - 1] : 0;
}

__device__ __forceinline__ uint32_t start_mask(const uint8_t (&b)[16], uint8_t prev, uint32_t i0, uint32_t n, int cr) {
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const uint8_t p = k ? b[k - 1] : prev;
        const bool s = i0 + k < n && (i0 + k == 0 || ends_line(p, b[k], cr));
        m |= uint32_t(s) << k;
    }
    return m;
}

__global__ __launch_bounds__(1024) void k_line_count(const uint8_t* __restrict__ text, uint32_t n, int cr, int* __restrict__ tile_cnt) {
    __shared__ long long wsum[17];
    const uint32_t i0 = blockIdx.x * uint32_t(LINE_TILE) + threadIdx.x * 16u;
    uint8_t b[16], prev;
    load16(text, n, i0, b, &prev);
    long long tot;
    (void)block_scan_excl(__popc(start_mask(b, prev, i0, n, cr)), &tot, wsum);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = int(tot);
}

__global__ __launch_bounds__(1024) void k_line_emit(const uint8_t* __restrict__ text, uint32_t n, int cr, const int* __restrict__ tile_base,
                                                    uint32_t* __restrict__ starts) {
    __shared__ long long wsum[17];
    const uint32_t i0 = blockIdx.x * uint32_t(LINE_TILE) + threadIdx.x * 16u;
    uint8_t b[16], prev;
    load16(text, n, i0, b, &prev);
    uint32_t m = start_mask(b, prev, i0, n, cr);
    long long tot;
    long long at = tile_base[blockIdx.x] + block_scan_excl(__popc(m), &tot, wsum);
    while (m) {
        const int k = __ffs(m) - 1;
        starts[at++] = i0 + uint32_t(k);
        m &= m - 1;
    }
}

}  // namespace
