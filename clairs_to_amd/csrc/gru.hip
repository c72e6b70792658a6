// BiGRU recurrent kernels (clairs/model.py:412-417, 442-448) - instantiations and launchers.
// Kept in a translation unit of their own so that edits to the CvT kernels cannot perturb their code generation.
#include "common.h"
#include "gru_kernel.h"
#include "gru_split_kernel.h"
#include "gru_tiles.h"

using namespace cto;

namespace {

int gru_cus() {      // compute units of the current device: one round of workgroups (gru_tiles.h)
    static const int cus = [] {
        int dev = 0, n = 256;
        if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
        return n > 0 ? n : 256;
    }();
    return cus;
}

// Wf / fc1f: the weights in fragment order (models.hip: pack_gru / pack_fc1_fragments).  XRAW: x is the address of the int16 tensor
template <int KIN, int KP, int H, int MS, bool FUSE, bool XRAW>
int launch_gru_range(hipStream_t s, const float* x, const float* Wf, const float* bias, float* out, const float* fc1f, float* fc1_part,
                     int64_t B, int64_t begin, int64_t end, const XRawArgs& raw) {
    const size_t smem = size_t(2) * MS * 16 * ((H + 4) + (KP + 4)) * sizeof(float);   // h tiles + x tiles
    static bool attr_set = false;
    if (!attr_set) {
        CTO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gru_layer_rot<KIN, KP, H, MS, FUSE, XRAW>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, int(smem)));
        attr_set = true;
    }
    const unsigned grid = unsigned(cdiv(end - begin, MS * 16)) * 2;
    hipLaunchKernelGGL((k_gru_layer_rot<KIN, KP, H, MS, FUSE, XRAW>), dim3(grid), dim3(256), smem, s, x, Wf, bias, out, fc1f, fc1_part, int(B),
                       int(begin), int(end), raw);
    CTO_HIP(hipGetLastError());
    return CTO_OK;
}

template <int KIN, int KP, int H, bool FUSE, bool XRAW = false>
int launch_gru(hipStream_t s, const float* x, const float* Wf, const float* bias, float* out, const float* fc1f, float* fc1_part, int64_t B,
               const XRawArgs& raw = XRawArgs{nullptr, 0, 0}) {
    return for_each_gru_tile_range(B, gru_cus(), [&](int64_t begin, int64_t end, auto ms) {
        return launch_gru_range<KIN, KP, H, decltype(ms)::value, FUSE, XRAW>(s, x, Wf, bias, out, fc1f, fc1_part, B, begin, end, raw);
    });
}

}  // namespace

// layer 1 on the int16 tensor, rescaled where the tile is staged (gru_kernel.h: XRAW)
int launch_gru_layer1_raw(hipStream_t s, const int16_t* x_raw, const int32_t* site_info, int which, int min_rescale_cov, const float* Wf,
                          const float* bias, float* out, int64_t B) {
    return launch_gru<34, 48, 128, false, true>(s, reinterpret_cast<const float*>(x_raw), Wf, bias, out, nullptr, nullptr, B,
                                                XRawArgs{site_info, which, min_rescale_cov});
}
int launch_gru_layer1(hipStream_t s, const float* x, const float* Wf, const float* bias, float* out, int64_t B) {
    return launch_gru<34, 48, 128, false>(s, x, Wf, bias, out, nullptr, nullptr, B);
}

// layer 2 with the head's fc1 folded in: writes one partial [B][128] slab per direction into fc1_part
int launch_gru_layer2_fc1(hipStream_t s, const float* x, const float* Wf, const float* bias, const float* fc1f, float* fc1_part, int64_t B) {
    return launch_gru<256, 256, 192, true>(s, x, Wf, bias, nullptr, fc1f, fc1_part, B);
}

// the recurrent layers on split 16-bit operands (experiment behind CTO_GRU_SPLIT=f16|bf16; gru_split_kernel.h): the same tile heights
template <int KIN, int KP, int H, int MS, bool F16, bool FUSE>
static int launch_split_range(hipStream_t s, const float* x, const void* Wp, const float* bias, const void* Fp, float* fc1_part,
                              float* out, int64_t B, int64_t begin, int64_t end, const GruSplitScale& sc) {
    const size_t smem = size_t(4) * MS * 16 * ((H + 8) + (KP + 8)) * sizeof(unsigned short) + size_t(4) * H * sizeof(float);
    static bool attr_set = false;
    if (!attr_set) {
        CTO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gru_split<KIN, KP, H, MS, F16, FUSE>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, int(smem)));
        attr_set = true;
    }
    const unsigned grid = unsigned(cdiv(end - begin, MS * 16)) * 2;
    hipLaunchKernelGGL((k_gru_split<KIN, KP, H, MS, F16, FUSE>), dim3(grid), dim3(256), smem, s, x, static_cast<const uint4*>(Wp), bias,
                       static_cast<const uint4*>(Fp), fc1_part, out, int(B), int(begin), int(end), sc);
    CTO_HIP(hipGetLastError());
    return CTO_OK;
}

template <int KIN, int KP, int H, bool F16, bool FUSE>
static int launch_split(hipStream_t s, const float* x, const void* Wp, const float* bias, const void* Fp, float* fc1_part, float* out,
                        int64_t B, const GruSplitScale& sc) {
    return for_each_gru_tile_range(B, gru_cus(), [&](int64_t begin, int64_t end, auto ms) {
        return launch_split_range<KIN, KP, H, decltype(ms)::value, F16, FUSE>(s, x, Wp, bias, Fp, fc1_part, out, B, begin, end, sc);
    });
}

// scale5 = {sx, sh, s_total, inv_s, inv_f} (GruSplitScale; chosen by pack_gru_split)
int launch_gru_layer2_fc1_split(hipStream_t s, const float* x, const void* Wp, const float* bias, const void* Fp, float* fc1_part,
                                int64_t B, bool f16, const float* scale5) {
    const GruSplitScale sc{scale5[0], scale5[1], scale5[2], scale5[3], scale5[4]};
    return f16 ? launch_split<256, 256, 192, true, true>(s, x, Wp, bias, Fp, fc1_part, nullptr, B, sc)
               : launch_split<256, 256, 192, false, true>(s, x, Wp, bias, Fp, fc1_part, nullptr, B, sc);
}

int launch_gru_layer1_split(hipStream_t s, const float* x, const void* Wp, const float* bias, float* out, int64_t B, bool f16,
                            const float* scale5) {
    const GruSplitScale sc{scale5[0], scale5[1], scale5[2], scale5[3], scale5[4]};
    return f16 ? launch_split<34, 64, 128, true, false>(s, x, Wp, bias, nullptr, nullptr, out, B, sc)
               : launch_split<34, 64, 128, false, false>(s, x, Wp, bias, nullptr, nullptr, out, B, sc);
}

#ifdef CTO_GRU_CLOCKS
extern "C" int cto_debug_gru_clocks(long long* out16) {
    CTO_HIP(hipDeviceSynchronize());
    CTO_HIP(hipMemcpyFromSymbol(out16, HIP_SYMBOL(cto::g_gru_clk), 16 * sizeof(long long)));
    return CTO_OK;
}
#endif
