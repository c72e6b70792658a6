// What the writers inside the library (csrc/contam.hip, csrc/bam.cpp) use of csrc/deflate.hip without going through the C ABI.
#pragma once
#include <vector>
#include "common.h"
#include "hip_buffers.h"

namespace cto {

// cto_bgzf_deflate's two paths; the counts and ms_kernels are added to *st (may be null)
int bgzf_deflate_device(const uint8_t* d_in, int64_t n, uint8_t* d_out, uint32_t* d_sizes, hipStream_t s, cto_deflate_stats* st);
int bgzf_deflate_host(const uint8_t* in, int64_t n, int threads, uint8_t* out, uint32_t* sizes, cto_deflate_stats* st);

// The device path for a writer on the host: the blocks of d_in[0 .. n) coded into d_slots, laid back to back in d_packed and copied
// down behind their sizes: h_down = uint32 sizes[n_blocks] (padded to 16 bytes) | the blocks' bytes.  Waits for the stream.
int bgzf_deflate_down(const uint8_t* d_in, int64_t n, hipStream_t s, DevBuf* d_slots, DevBuf* d_packed, PinBuf* h_down, const uint32_t** sizes,
                      const uint8_t** bytes, int64_t* n_bytes, cto_deflate_stats* st, double* ms_copy);
// the same for bytes on the host: copied up, coded, the blocks back to back in *bytes
int bgzf_deflate_updown(const uint8_t* h_in, int64_t n, hipStream_t s, std::vector<uint8_t>* bytes, std::vector<uint32_t>* sizes, cto_deflate_stats* st);

}  // namespace cto
