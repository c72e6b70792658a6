// Test-only entry points onto the three headers that every device command rests on: the prefix sums of scan.h, the line starts of lines.h
// and the constants of sort.h (cto_sort_u64, the sort alone, lives in addback.hip).  Nothing command-specific is included.
//
// The kernels of those headers sit in anonymous namespaces, so this file compiles its OWN copy of them, as each of their users does
// (pileup, extract, allelecount, aftally, hapwindows, phase, contam, pon, addback, comparevcf): what is tested here is the source text
// the users share, launched as they launch it, not the users' object code.  tests/test_gpu_primitives.py therefore also goes through
// cto_candidate_positions and cto_add_back at the sizes that cross the same seams.
//
// Every entry takes `where`: 0 runs the kernels on `stream`, 1 a plain sequential loop on the host that shares nothing with them and
// states what the operation is.  Arrays are the caller's, on the host.
#include <mutex>
#include "hip_buffers.h"
#include "lines.h"
#include "sort.h"

using namespace cto;

namespace {

struct PrimCtx {
    std::mutex mu;
    DevBuf in, in2, out, out2, total, tile_tmp, tile_tot;         // the scans
    DevBuf tiles_a, tiles_tot;                                     // the tile scan
    DevBuf text, tiles, tile_base, line_tmp, line_tot, starts;     // the line starts
    void release() {
        for (DevBuf* b : {&in, &in2, &out, &out2, &total, &tile_tmp, &tile_tot, &tiles_a, &tiles_tot, &text, &tiles, &tile_base, &line_tmp, &line_tot, &starts}) {
            if (b->p) (void)hipFree(b->p);
            b->p = nullptr;
            b->cap = 0;
        }
    }
};

#define PRIM_LAUNCH_OK(what)                                                                    \
    do {                                                                                        \
        const hipError_t le__ = hipGetLastError();                                              \
        CTO_REQUIRE(le__ == hipSuccess, CTO_EHIP, "%s: %s", what, hipGetErrorString(le__));     \
    } while (0)

template <typename Out>
void scan_host(const int32_t* in, int64_t n, Out* out, Out* total) {
    long long sum = 0;
    for (int64_t i = 0; i < n; ++i) { out[i] = Out(sum); sum += in[i]; }
    out[n] = Out(sum);
    if (total) *total = Out(sum);
}

// one array after the other on the same stream and the same tile scratch; results copied back behind both
template <typename Out>
int scan_device(PrimCtx& x, hipStream_t s, const int32_t* in, const int32_t* in2, int n, int form, Out* out, Out* out2, Out* total) {
    const size_t N = size_t(n), out_bytes = (N + 1) * sizeof(Out);
    int rc;
    if ((rc = x.in.ensure(N * 4 + 4)) || (rc = x.out.ensure(out_bytes)) || (rc = x.total.ensure(2 * sizeof(Out))) ||
        (rc = x.tile_tmp.ensure((N / SCAN_TILE + 8) * sizeof(long long))) || (rc = x.tile_tot.ensure(sizeof(long long))))
        return rc;
    if (in2 && ((rc = x.in2.ensure(N * 4 + 4)) || (rc = x.out2.ensure(out_bytes)))) return rc;
    const int32_t* src[2] = {in, in2};
    Out* dst[2] = {out, out2};
    DevBuf* d_in[2] = {&x.in, &x.in2};
    DevBuf* d_out[2] = {&x.out, &x.out2};
    Out* d_total = total ? x.total.as<Out>() : nullptr;
    if (d_total) CTO_HIP(hipMemsetAsync(d_total, 0xA5, 2 * sizeof(Out), s));
    for (int k = 0; k < 2; ++k) {
        if (!src[k]) continue;
        Out* tot = d_total ? d_total + k : nullptr;
        if (form == 1) {                                    // in place, as cto_candidate_positions scans its block counts (Out is int32_t here)
            int32_t* a = d_out[k]->as<int32_t>();
            if (n) CTO_HIP(hipMemcpyAsync(a, src[k], N * 4, hipMemcpyHostToDevice, s));
            CTO_HIP(hipMemsetAsync(a + n, 0xA5, 4, s));
            hipLaunchKernelGGL(k_scan_small<int32_t>, dim3(1), dim3(1024), 0, s, a, a, n, reinterpret_cast<int32_t*>(tot));
        } else {
            if (n) CTO_HIP(hipMemcpyAsync(d_in[k]->p, src[k], N * 4, hipMemcpyHostToDevice, s));
            CTO_HIP(hipMemsetAsync(d_out[k]->p, 0xA5, out_bytes, s));       // what no kernel writes does not look like an earlier call's result
            scan_exclusive<Out>(s, d_in[k]->as<int>(), n, d_out[k]->as<Out>(), tot, x.tile_tmp.as<long long>(), x.tile_tot.as<long long>());
        }
    }
    PRIM_LAUNCH_OK("cto_prim_scan");
    for (int k = 0; k < 2; ++k)
        if (src[k]) CTO_HIP(hipMemcpyAsync(dst[k], d_out[k]->p, out_bytes, hipMemcpyDeviceToHost, s));
    if (total) CTO_HIP(hipMemcpyAsync(total, d_total, (in2 ? 2 : 1) * sizeof(Out), hipMemcpyDeviceToHost, s));
    CTO_HIP(hipStreamSynchronize(s));
    return CTO_OK;
}

template <typename Out>
int scan_any(const int32_t* in, const int32_t* in2, int64_t n, int form, int where, void* stream, void* out, void* out2, void* total) {
    Out* t = static_cast<Out*>(total);
    if (where == 1) {
        scan_host<Out>(in, n, static_cast<Out*>(out), t);
        if (in2) scan_host<Out>(in2, n, static_cast<Out*>(out2), t ? t + 1 : nullptr);
        return CTO_OK;
    }
    PrimCtx& x = process_wide<PrimCtx>();
    std::lock_guard<std::mutex> lock(x.mu);
    return scan_device<Out>(x, static_cast<hipStream_t>(stream), in, in2, int(n), form, static_cast<Out*>(out), static_cast<Out*>(out2), t);
}

bool starts_line(const uint8_t* t, int64_t i, int cr) {
    if (i == 0) return true;
    return t[i - 1] == '\n' || (cr && t[i - 1] == '\r' && t[i] != '\n');
}

}  // namespace

extern "C" int cto_prim_constants(int64_t* out) {
    CTO_REQUIRE(out, CTO_EINVAL, "cto_prim_constants: a null pointer");
    out[0] = SCAN_TILE;
    out[1] = SORT_TILE;
    out[2] = LINE_TILE;
    out[3] = SORT_MAX_N;
    return CTO_OK;
}

extern "C" int cto_prim_scan(const int32_t* in, const int32_t* in2, int64_t n, int out_bits, int form, int where, void* stream, void* out, void* out2,
                             void* total) try {
    CTO_REQUIRE(n >= 0 && n < (int64_t(1) << 30) && out && (n == 0 || in) && (!in2 || out2), CTO_EINVAL, "cto_prim_scan: a null pointer or n outside 0 .. 2^30 - 1");
    CTO_REQUIRE((out_bits == 32 || out_bits == 64) && (form == 0 || (form == 1 && out_bits == 32)) && (where == 0 || where == 1), CTO_EINVAL,
                "cto_prim_scan: out_bits is 32 or 64, form 0 or (with 32 bits) 1, where 0 or 1");
    return out_bits == 32 ? scan_any<int32_t>(in, in2, n, form, where, stream, out, out2, total)
                          : scan_any<long long>(in, in2, n, form, where, stream, out, out2, total);
} CTO_CATCH("cto_prim_scan", int)

extern "C" int cto_prim_scan_tiles(int64_t* a, int64_t n, int stride, int where, void* stream, int64_t* totals) try {
    CTO_REQUIRE(n >= 0 && n < (int64_t(1) << 24) && (n == 0 || a) && totals && stride >= 1 && stride <= 3 && (where == 0 || where == 1), CTO_EINVAL,
                "cto_prim_scan_tiles: a null pointer, n outside 0 .. 2^24 - 1, a stride outside 1 .. 3 or another `where`");
    if (where == 1) {
        for (int j = 0; j < stride; ++j) {
            int64_t sum = 0;
            for (int64_t i = 0; i < n; ++i) { const int64_t v = a[i * stride + j]; a[i * stride + j] = sum; sum += v; }
            totals[j] = sum;
        }
        return CTO_OK;
    }
    PrimCtx& x = process_wide<PrimCtx>();
    std::lock_guard<std::mutex> lock(x.mu);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t bytes = size_t(n) * size_t(stride) * 8;
    int rc;
    if ((rc = x.tiles_a.ensure(bytes + 8)) || (rc = x.tiles_tot.ensure(64))) return rc;
    if (bytes) CTO_HIP(hipMemcpyAsync(x.tiles_a.p, a, bytes, hipMemcpyHostToDevice, s));
    CTO_HIP(hipMemsetAsync(x.tiles_tot.p, 0xA5, 64, s));
    hipLaunchKernelGGL(k_scan_tiles, dim3(1), dim3(1024), 0, s, x.tiles_a.as<long long>(), int(n), stride, x.tiles_tot.as<long long>());
    PRIM_LAUNCH_OK("cto_prim_scan_tiles");
    if (bytes) CTO_HIP(hipMemcpyAsync(a, x.tiles_a.p, bytes, hipMemcpyDeviceToHost, s));
    CTO_HIP(hipMemcpyAsync(totals, x.tiles_tot.p, size_t(stride) * 8, hipMemcpyDeviceToHost, s));
    CTO_HIP(hipStreamSynchronize(s));
    return CTO_OK;
} CTO_CATCH("cto_prim_scan_tiles", int)

extern "C" int64_t cto_prim_line_starts(const uint8_t* text, int64_t n, int cr, int where, void* stream, uint32_t* starts, int64_t cap) try {
    CTO_REQUIRE(n >= 0 && (n == 0 || text) && cap >= 0 && (cap == 0 || starts) && (cr == 0 || cr == 1) && (where == 0 || where == 1), CTO_EINVAL,
                "cto_prim_line_starts: a null pointer, a negative length, or cr or where that is not 0 or 1");
    CTO_REQUIRE(n < (int64_t(1) << 32) - LINE_TILE, CTO_EUNSUPPORTED, "cto_prim_line_starts: 4 GB of text or more");
    if (n == 0) return 0;
    if (where == 1) {
        int64_t count = 0;
        for (int64_t i = 0; i < n; ++i) count += starts_line(text, i, cr);
        if (count > cap) return count;
        int64_t at = 0;
        for (int64_t i = 0; i < n; ++i) if (starts_line(text, i, cr)) starts[at++] = uint32_t(i);
        return count;
    }
    PrimCtx& x = process_wide<PrimCtx>();
    std::lock_guard<std::mutex> lock(x.mu);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t T = size_t(n), padded = align16(T) + 16;          // hipMalloc aligns to more than 16 bytes; zeros behind the text
    const int tiles = int(cdiv(n, LINE_TILE));
    int rc;
    if ((rc = x.text.ensure(padded)) || (rc = x.tiles.ensure(sizeof(int) * size_t(tiles))) || (rc = x.tile_base.ensure(sizeof(int) * size_t(tiles + 1))) ||
        (rc = x.line_tmp.ensure(sizeof(long long) * size_t(cdiv(tiles, SCAN_TILE) + 1))) || (rc = x.line_tot.ensure(sizeof(long long))))
        return rc;
    uint8_t* d_text = x.text.as<uint8_t>();
    CTO_HIP(hipMemcpyAsync(d_text, text, T, hipMemcpyHostToDevice, s));
    CTO_HIP(hipMemsetAsync(d_text + T, 0, padded - T, s));
    hipLaunchKernelGGL(k_line_count, dim3(unsigned(tiles)), dim3(1024), 0, s, d_text, uint32_t(T), cr, x.tiles.as<int>());
    scan_exclusive<int>(s, x.tiles.as<int>(), tiles, x.tile_base.as<int>(), nullptr, x.line_tmp.as<long long>(), x.line_tot.as<long long>());
    PRIM_LAUNCH_OK("cto_prim_line_starts: line counts");
    int n_lines = 0;
    CTO_HIP(hipMemcpyAsync(&n_lines, x.tile_base.as<int>() + tiles, sizeof(int), hipMemcpyDeviceToHost, s));
    CTO_HIP(hipStreamSynchronize(s));
    CTO_REQUIRE(n_lines >= 0 && int64_t(n_lines) <= n, CTO_EHIP, "cto_prim_line_starts: %d line starts in %lld bytes", n_lines, (long long)n);
    if (n_lines > cap) return n_lines;
    if ((rc = x.starts.ensure(sizeof(uint32_t) * size_t(n_lines + 1)))) return rc;
    CTO_HIP(hipMemsetAsync(x.starts.p, 0xA5, sizeof(uint32_t) * size_t(n_lines + 1), s));
    hipLaunchKernelGGL(k_line_emit, dim3(unsigned(tiles)), dim3(1024), 0, s, d_text, uint32_t(T), cr, x.tile_base.as<int>(), x.starts.as<uint32_t>());
    PRIM_LAUNCH_OK("cto_prim_line_starts: line starts");
    if (n_lines) CTO_HIP(hipMemcpyAsync(starts, x.starts.p, sizeof(uint32_t) * size_t(n_lines), hipMemcpyDeviceToHost, s));
    CTO_HIP(hipStreamSynchronize(s));
    return n_lines;
} CTO_CATCH("cto_prim_line_starts", int64_t)

// frees the device buffers the entries above keep from call to call, so that the next calls grow them again from nothing
extern "C" int cto_prim_release(void) {
    PrimCtx& x = process_wide<PrimCtx>();
    std::lock_guard<std::mutex> lock(x.mu);
    x.release();
    return CTO_OK;
}
