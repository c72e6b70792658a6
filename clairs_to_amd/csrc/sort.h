// Stable sort of (64-bit key, 32-bit payload) pairs by key (addback.hip; cto_sort_u64): a least-significant-digit radix sort, 8 bits a
// pass, on the device and - the same passes, one thread - on the host.
//
// One pass over a digit is three steps: k_sort_hist counts each tile's keys per digit value (hist[value * tiles + tile]), scan_exclusive
// (scan.h) over that table gives every (value, tile) its first output slot, and k_sort_scatter moves the pairs.  A tile is 2048 pairs, four
// waves of 64 lanes with 8 pairs a lane; wave w owns pairs [512 w, 512 w + 512) of the tile and takes them 64 at a time, in order.
// The rank of a pair among the pairs of its digit value is
//     the slot of (value, tile)  +  the pairs of that value in the waves before  +  those in the wave's earlier rounds
//     +  the lanes below it in the round that hold the same value,
// and the last term comes from eight wave ballots, one per bit of the digit (64 bits wide on gfx950): the lanes whose ballots agree with
// this lane's bit in all eight are its peers.  No atomic decides a position, so equal keys keep their input order and the result is unique.
// Digits in which no two keys differ (`varying`, the OR of the keys XOR their AND, or any superset the caller knows) are skipped.
// In an anonymous namespace: every translation unit that includes it has its own kernels.
#pragma once
#include <vector>
#include "hip_buffers.h"
#include "scan.h"

namespace {

constexpr int SORT_THREADS = 256, SORT_ITEMS = 8, SORT_WAVES = SORT_THREADS / 64;
constexpr int SORT_TILE = SORT_THREADS * SORT_ITEMS;   // 2048 pairs per workgroup
constexpr int64_t SORT_MAX_N = int64_t(1) << 30;       // slots are ints, and the histogram table (256 x tiles) is scanned as ints

__global__ __launch_bounds__(SORT_THREADS) void k_sort_hist(const uint64_t* __restrict__ keys, int64_t n, int shift, int tiles, int* __restrict__ hist) {
    __shared__ int cnt[256];
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const int64_t e0 = int64_t(blockIdx.x) * SORT_TILE + threadIdx.x;
#pragma unroll
    for (int it = 0; it < SORT_ITEMS; ++it) {
        const int64_t e = e0 + int64_t(it) * SORT_THREADS;
        if (e < n) atomicAdd(&cnt[int(keys[e] >> shift) & 255], 1);          // a count: the order of the additions does not show
    }
    __syncthreads();
    hist[size_t(threadIdx.x) * tiles + blockIdx.x] = cnt[threadIdx.x];
}

__global__ __launch_bounds__(SORT_THREADS) void k_sort_scatter(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ pay,
                                                               uint64_t* __restrict__ keys_out, uint32_t* __restrict__ pay_out, int64_t n, int shift,
                                                               int tiles, const int* __restrict__ slot) {
    __shared__ int cnt[SORT_WAVES][256];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
#pragma unroll
    for (int w = 0; w < SORT_WAVES; ++w) cnt[w][t] = 0;
    __syncthreads();
    const int64_t e0 = int64_t(blockIdx.x) * SORT_TILE + int64_t(wave) * (64 * SORT_ITEMS) + lane;
    const uint64_t below = (uint64_t(1) << lane) - 1;
    uint64_t k[SORT_ITEMS];
    int local[SORT_ITEMS];
#pragma unroll
    for (int it = 0; it < SORT_ITEMS; ++it) {
        const int64_t e = e0 + it * 64;
        const bool valid = e < n;
        k[it] = valid ? keys[e] : 0;
        const int d = int(k[it] >> shift) & 255;
        uint64_t peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1;
            const uint64_t m = __ballot(valid && bit);
            peers &= bit ? m : ~m;
        }
        const int before = __popcll(peers & below);
        const int base = cnt[wave][d];
        __syncthreads();                                  // every lane has read its counter before the round's first peer moves it on
        if (valid && before == 0) cnt[wave][d] = base + __popcll(peers);
        __syncthreads();
        local[it] = base + before;
    }
    {                                                     // per value: the tile's slot, then wave after wave
        int run = slot[size_t(t) * tiles + blockIdx.x];
#pragma unroll
        for (int w = 0; w < SORT_WAVES; ++w) { const int c = cnt[w][t]; cnt[w][t] = run; run += c; }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < SORT_ITEMS; ++it) {
        const int64_t e = e0 + it * 64;
        if (e < n) {
            const int at = cnt[wave][int(k[it] >> shift) & 255] + local[it];
            keys_out[at] = k[it];
            pay_out[at] = pay[e];
        }
    }
}

struct SortScratch {
    cto::DevBuf hist, slot, tile_tmp, tile_tot;
    int ensure(int64_t n) {
        const size_t cells = size_t(256) * size_t(cto::cdiv(n > 0 ? n : 1, SORT_TILE));
        int rc;
        if ((rc = hist.ensure(cells * sizeof(int))) || (rc = slot.ensure((cells + 1) * sizeof(int)))) return rc;
        if ((rc = tile_tmp.ensure((size_t(cto::cdiv(int64_t(cells), SCAN_TILE)) + 1) * sizeof(long long)))) return rc;
        return tile_tot.ensure(sizeof(long long));
    }
};

// Sorts the n pairs in (ka, pa) on stream s, with (kb, pb) as the other half of the ping-pong; *in_b = 1 when the result is in (kb, pb).
// Launch errors are the caller's to collect.
inline int sort_pairs_device(hipStream_t s, uint64_t* ka, uint32_t* pa, uint64_t* kb, uint32_t* pb, int64_t n, uint64_t varying, SortScratch& sc,
                             int* in_b) {
    *in_b = 0;
    if (n < 2) return CTO_OK;
    CTO_REQUIRE(n <= SORT_MAX_N, CTO_EUNSUPPORTED, "sort: more than 2^30 pairs");
    int rc;
    if ((rc = sc.ensure(n))) return rc;
    const int tiles = int(cto::cdiv(n, SORT_TILE));
    for (int shift = 0; shift < 64; shift += 8) {
        if (((varying >> shift) & 255) == 0) continue;
        const uint64_t* ki = *in_b ? kb : ka;
        const uint32_t* pi = *in_b ? pb : pa;
        hipLaunchKernelGGL(k_sort_hist, dim3(unsigned(tiles)), dim3(SORT_THREADS), 0, s, ki, n, shift, tiles, sc.hist.as<int>());
        scan_exclusive<int>(s, sc.hist.as<int>(), 256 * tiles, sc.slot.as<int>(), nullptr, sc.tile_tmp.as<long long>(), sc.tile_tot.as<long long>());
        hipLaunchKernelGGL(k_sort_scatter, dim3(unsigned(tiles)), dim3(SORT_THREADS), 0, s, ki, pi, *in_b ? ka : kb, *in_b ? pa : pb, n, shift, tiles,
                           sc.slot.as<int>());
        *in_b ^= 1;
    }
    return CTO_OK;
}

// the same passes on the host, in place
inline void sort_pairs_host(uint64_t* keys, uint32_t* pay, int64_t n, uint64_t varying) {
    if (n < 2) return;
    std::vector<uint64_t> k2(static_cast<size_t>(n));
    std::vector<uint32_t> p2(static_cast<size_t>(n));
    uint64_t *ki = keys, *ko = k2.data();
    uint32_t *pi = pay, *po = p2.data();
    for (int shift = 0; shift < 64; shift += 8) {
        if (((varying >> shift) & 255) == 0) continue;
        int64_t at[257] = {0};
        for (int64_t i = 0; i < n; ++i) ++at[((ki[i] >> shift) & 255) + 1];
        for (int d = 0; d < 256; ++d) at[d + 1] += at[d];
        for (int64_t i = 0; i < n; ++i) {
            const int64_t o = at[(ki[i] >> shift) & 255]++;
            ko[o] = ki[i];
            po[o] = pi[i];
        }
        std::swap(ki, ko);
        std::swap(pi, po);
    }
    if (ki != keys) {
        memcpy(keys, ki, size_t(n) * sizeof(uint64_t));
        memcpy(pay, pi, size_t(n) * sizeof(uint32_t));
    }
}

inline uint64_t varying_bits(const uint64_t* keys, int64_t n) {
    uint64_t o = 0, a = ~uint64_t(0);
    for (int64_t i = 0; i < n; ++i) { o |= keys[i]; a &= keys[i]; }
    return n ? o ^ a : 0;
}

}  // namespace
