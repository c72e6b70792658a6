// BGZF deflate on the device: the counterpart of inflate.hip for the BAMs this package writes (gen_contaminated_bam's mix,
// phase_tumor's haplotagged BAM, bgzf.deflate_bytes).  cto_bgzf_deflate is the C entry point.  The reference starts samtools / bgzip for
// this, so there is nothing to be equal to but DEFLATE itself: the rules below are the definition, csrc/deflate_host.h states them as
// plain sequential C++ (the host path, `where` 1), and the kernel is held equal to it byte for byte (tests/test_gpu_bgzf_deflate.py).
// Every function both sides need - the match of a position, the walk of a segment, the code construction, the plan of a block, the
// bit writer - is one text in deflate_host.h compiled for both.
//
// Rules.  All arithmetic is integer; the output is a pure function of the input bytes.
//   1. Blocks.  The input is cut every 0xff00 bytes (the last block shorter); block b becomes one whole BGZF block in out + b * 65536:
//      the 18-byte header with BSIZE, one RFC 1951 block with BFINAL = 1, CRC-32 and ISIZE.  n == 0 gives no block.  Everything below is
//      per block: d[0 .. n), positions p.
//   2. Segments.  The block is cut every SEG = 512 bytes into segments.  A token never crosses a segment's end, so the segments are
//      parsed independently of one another (one lane each); a match may still copy from any earlier segment.
//   3. The match at p.  max_len = min(258, segment end - p); below 3 there is none.  Candidates q are
//        - the table's: the largest q' < 256 * floor(p / 256) (the start of p's tile of 256 positions) with q' + 4 <= n and
//          hash(d[q' .. q' + 4)) == hash(d[p .. p + 4)), if p + 4 <= n; hash(v) = (v * 2654435761 mod 2^32) >> 18 of the four bytes
//          as a little-endian number (a candidate is a candidate whether its bytes are equal or only its hash);
//        - p - 1, p - 2, p - 3, p - 4, p - 6, p - 8, where not negative (the table does not see inside p's own tile; these catch runs
//          of qualities and homopolymers and short repeats in the packed bases);
//      each with 1 <= p - q <= 32768.  Its length is the number of equal bytes d[q + i] == d[p + i], i < max_len (q + i may reach past
//      p: an overlapping copy).  The longest wins, the smaller distance among equal lengths.  It is a match if its length is at least
//      4, or 3 with a distance of at most 4096.
//   4. Tokens.  Each segment is walked from its start: a match at p is taken whole and the walk goes on behind it (greedy, no lazy
//      evaluation), otherwise d[p] is a literal.  The block's tokens are the segments' tokens in order, then end-of-block.
//   5. Codes.  hist = how often each of the 286 literal/length and 30 distance symbols occurs (end-of-block once).
//      a. In either alphabet with fewer than two used symbols the unused ones among symbols 0, 1, 2 get frequency 1 in turn until two
//         are used (zlib's build_tree does the like): every decoder accepts the code.
//      b. Lengths: the used symbols ascending by (frequency, symbol) are the leaves of a Huffman tree built with two queues, a leaf
//         before an inner node of the same weight.  Depths beyond the limit (15; 7 for the code-length code) count as the limit; while
//         the Kraft sum exceeds 1 one leaf leaves the deepest level and one leaf of the deepest level above that still has one goes a
//         level down beside it.  The counts per length are then dealt out in the sorted order, the longest to the rarest.  Where
//         the unlimited tree fits, the lengths are optimal.
//      c. The header: HLIT and HDIST end at the last used symbol (at least 257 and 1); the lengths of both alphabets as one sequence,
//         a run of zeros as 18 (11 .. 138, the longest first) then 17 (3 .. 10) then single zeros, a run of another length as the length
//         itself then 16 (3 .. 6, the longest first) then the length again; the code-length code by a and b from these symbols.
//   6. Type.  bits[stored] = 8 * (n + 5); bits[fixed] and bits[dynamic] = 3 + the header (dynamic: 14 + 3 * HCLEN + the coded
//      lengths) + the tokens under that code with their extra bits.  The type with the fewest bits, on a tie stored before fixed before
//      dynamic; stored as well when ceil(bits / 8) would exceed 65536 - 26.  The payload has ceil(bits / 8) bytes, so a block has
//      at most n + 31.
//   7. Bits go out as RFC 1951 orders them: codes from their most significant bit, everything else from the least, bytes filled
//      from bit 0.
//
// Device path.  k_crc32_values (bam_records.h: one wave per block, the slice-and-chain CRC of the readers) first, then
//   k_deflate      one workgroup of 256 lanes per block, as many workgroups as the device has CUs (each takes blocks in turn).  LDS:
//                  the block (65280 B), a table of 2^14 positions (64 KiB), the histogram, the scratch and the plan: 141 KiB, hence
//                  one workgroup per CU and dynamic LDS.
//                  matches   tile by tile, one lane per position: look the table up and find the match (rule 3), barrier, atomicMax of
//                            p + 1 into the slot, barrier - so a slot holds the largest earlier position whatever order the lanes
//                            run in.  The matches go to a scratch array in device memory (4 bytes per position, one array per
//                            workgroup): the three walks below read them back instead of comparing bytes again.
//                  walk A    one lane per segment: the histogram, atomicAdd in LDS.
//                  codes     frequencies with the forced pair; the (frequency, symbol) order by ranking, one lane per symbol; then
//                            one lane builds the lengths, the header and the three sizes (plan_block).
//                  walk B    per segment the bits of its tokens under the chosen code; one lane scans them into bit offsets.
//                  walk C    every lane ORs its tokens into the output staged in LDS (the table's 64 KiB, zeroed: atomicOr, so shared
//                            words do not depend on order); lane 0 the header and end-of-block.  The payload and the frame go out.
//   k_pack_*       for a writer on the host: the blocks back to back, so that only compressed bytes come down.
// Measured and rejected: see DESIGN.md section 3.
#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>
#include "bam_records.h"
#include "common.h"
#include "deflate_host.h"
#include "deflate_internal.h"
#include "hip_buffers.h"
#include "pack_internal.h"

using namespace cto;
namespace df = cto::dfl;

namespace {

static_assert(df::kSeg >= 256, "one lane per segment: a block has at most 256 segments");
static_assert(df::kPayload == CTO_BGZF_PAYLOAD, "the block cut of the header");

constexpr int kDataBytes = df::kPayload + 16;
constexpr int kTableBytes = 4 << df::kHashBits;
struct Small {
    uint32_t hist[df::kHist + 4];
    df::HuffWs ws;
    df::Plan pl;
    uint32_t seg_bits[256];
};
constexpr size_t kLdsBytes = size_t(kDataBytes) + kTableBytes + sizeof(Small);
static_assert(kLdsBytes <= 160 * 1024, "LDS of a CU");

struct DbgOut { long long bits[3]; uint32_t hist[df::kHist]; };

__global__ __launch_bounds__(256) void k_deflate(const uint8_t* __restrict__ in, int64_t n, int n_blocks, const uint32_t* __restrict__ crc,
                                                 uint32_t* __restrict__ gmatch, uint8_t* __restrict__ out, uint32_t* __restrict__ sizes,
                                                 unsigned long long* __restrict__ counts, DbgOut* dbg) {
    extern __shared__ __align__(16) uint8_t lds[];
    uint8_t* const data = lds;
    uint32_t* const table = reinterpret_cast<uint32_t*>(lds + kDataBytes);
    Small* const S = reinterpret_cast<Small*>(lds + kDataBytes + kTableBytes);
    uint32_t* const match = gmatch + size_t(blockIdx.x) * df::kPayload;
    const int tid = threadIdx.x;
    for (int b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const uint8_t* src = in + int64_t(b) * df::kPayload;
        const int nb = int(min(int64_t(df::kPayload), n - int64_t(b) * df::kPayload));
        if ((reinterpret_cast<uintptr_t>(src) & 3) == 0) {
            const int nw = nb >> 2;
            for (int i = tid; i < nw; i += 256) reinterpret_cast<uint32_t*>(data)[i] = reinterpret_cast<const uint32_t*>(src)[i];
            for (int i = (nw << 2) + tid; i < nb; i += 256) data[i] = src[i];
        } else {
            for (int i = tid; i < nb; i += 256) data[i] = src[i];
        }
        for (int i = tid; i < (1 << df::kHashBits); i += 256) table[i] = 0;
        for (int i = tid; i < df::kHist; i += 256) S->hist[i] = 0;
        __syncthreads();
        // rule 3: a slot holds 1 + the largest position of the earlier tiles with its hash
        for (int t0 = 0; t0 < nb; t0 += df::kTile) {
            const int p = t0 + tid;
            const bool hashed = p + 4 <= nb;
            uint32_t h = 0;
            if (p < nb) {
                if (hashed) h = df::hash4(data + p);
                match[p] = df::match_at(data, nb, p, hashed ? int(table[h]) - 1 : -1);
            }
            __syncthreads();
            if (hashed) atomicMax(&table[h], uint32_t(p + 1));
            __syncthreads();
        }
        const int n_seg = (nb + df::kSeg - 1) / df::kSeg;
        if (tid < n_seg)
            df::walk_segment(data, match, nb, tid, [&](int len, int v) {
                if (!len) { atomicAdd(&S->hist[v], 1u); return; }
                int ls, le, lv, ds, de, dv;
                df::length_code(len, &ls, &le, &lv);
                df::dist_code(v, &ds, &de, &dv);
                atomicAdd(&S->hist[ls], 1u);
                atomicAdd(&S->hist[df::kNumLL + ds], 1u);
            });
        if (tid == 0) atomicAdd(&S->hist[256], 1u);
        __syncthreads();
        for (int s = tid; s < 288; s += 256) S->ws.f_ll[s] = s < df::kNumLL ? S->hist[s] : 0;
        if (tid < 32) S->ws.f_d[tid] = tid < df::kNumD ? S->hist[df::kNumLL + tid] : 0;
        __syncthreads();
        if (tid == 0) { df::force_pair(S->ws.f_ll, df::kNumLL); df::force_pair(S->ws.f_d, df::kNumD); }
        __syncthreads();
        for (int s = tid; s < df::kNumLL; s += 256) {
            int r = 0;
            for (int j = 0; j < df::kNumLL; ++j) r += df::freq_less(S->ws.f_ll, j, s);
            S->ws.ord_ll[r] = uint16_t(s);
        }
        if (tid < df::kNumD) {
            int r = 0;
            for (int j = 0; j < df::kNumD; ++j) r += df::freq_less(S->ws.f_d, j, tid);
            S->ws.ord_d[r] = uint16_t(tid);
        }
        __syncthreads();
        if (tid == 0) df::plan_block(S->hist, nb, &S->ws, &S->pl);
        __syncthreads();
        const int type = S->pl.type;
        const int clen = type == 0 ? nb + 5 : int((S->pl.bits[type] + 7) / 8);
        uint8_t* const o = out + size_t(b) * df::kSlot;
        if (type == 0) {
            if (tid == 0) { o[18] = 1; o[19] = uint8_t(nb); o[20] = uint8_t(nb >> 8); o[21] = uint8_t(~nb); o[22] = uint8_t((~nb) >> 8); }
            for (int i = tid; i < nb; i += 256) o[23 + i] = data[i];
        } else {
            for (int i = tid; i < (1 << df::kHashBits); i += 256) table[i] = 0;
            if (tid < n_seg) {
                uint32_t bits = 0;
                df::walk_segment(data, match, nb, tid, [&](int len, int v) { bits += uint32_t(df::token_bits(&S->pl, len, v)); });
                S->seg_bits[tid] = bits;
            }
            __syncthreads();
            auto or_word = [&](uint32_t i, uint32_t x) { atomicOr(&table[i], x); };
            if (tid == 0) {
                uint32_t at = df::put_header(or_word, &S->pl);
                for (int s = 0; s < n_seg; ++s) { const uint32_t t = S->seg_bits[s]; S->seg_bits[s] = at; at += t; }
                df::put_bits(or_word, &at, S->pl.e_ll_code[256], S->pl.e_ll_len[256]);
            }
            __syncthreads();
            if (tid < n_seg) {
                uint32_t pos = S->seg_bits[tid];
                df::walk_segment(data, match, nb, tid, [&](int len, int v) { df::put_token(or_word, &pos, &S->pl, len, v); });
            }
            __syncthreads();
            const uint8_t* staged = reinterpret_cast<const uint8_t*>(table);
            for (int i = tid; i < clen; i += 256) o[18 + i] = staged[i];
        }
        if (tid == 0) {
            df::bgzf_frame(o, clen, crc[b], uint32_t(nb));
            sizes[b] = uint32_t(clen + 26);
            atomicAdd(&counts[type], 1ull);
            atomicAdd(&counts[3], (unsigned long long)(clen + 26));
            if (dbg) {
                for (int k = 0; k < 3; ++k) dbg->bits[k] = S->pl.bits[k];
                for (int k = 0; k < df::kHist; ++k) dbg->hist[k] = S->hist[k];
            }
        }
        __syncthreads();
    }
}

// rule 5 a/b alone, for the test seam: one workgroup, the alphabet in LDS
__global__ __launch_bounds__(256) void k_code_lengths(const uint32_t* __restrict__ freq, int n_sym, int max_bits, uint8_t* __restrict__ len) {
    __shared__ df::HuffWs ws;
    __shared__ uint8_t out[288];
    const int tid = threadIdx.x;
    for (int s = tid; s < 288; s += 256) ws.f_ll[s] = s < n_sym ? freq[s] : 0;
    __syncthreads();
    if (tid == 0) df::force_pair(ws.f_ll, n_sym);
    __syncthreads();
    for (int s = tid; s < n_sym; s += 256) {
        int r = 0;
        for (int j = 0; j < n_sym; ++j) r += df::freq_less(ws.f_ll, j, s);
        ws.ord_ll[r] = uint16_t(s);
    }
    __syncthreads();
    if (tid == 0) df::build_lengths(ws.f_ll, n_sym, ws.ord_ll, max_bits, &ws, out);
    __syncthreads();
    for (int s = tid; s < n_sym; s += 256) len[s] = out[s];
}

// the blocks of the slots back to back: offsets by one lane (a window has a few thousand blocks at most), then one workgroup per block
__global__ void k_pack_offsets(const uint32_t* __restrict__ sizes, int n_blocks, unsigned long long* __restrict__ off) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        unsigned long long at = 0;
        for (int b = 0; b < n_blocks; ++b) { off[b] = at; at += sizes[b]; }
        off[n_blocks] = at;
    }
}
__global__ __launch_bounds__(256) void k_pack_copy(const uint8_t* __restrict__ slots, const uint32_t* __restrict__ sizes,
                                                   const unsigned long long* __restrict__ off, uint8_t* __restrict__ packed) {
    const uint8_t* s = slots + size_t(blockIdx.x) * df::kSlot;
    uint8_t* d = packed + off[blockIdx.x];
    const uint32_t n = sizes[blockIdx.x];
    for (uint32_t i = threadIdx.x; i < n; i += 256) d[i] = s[i];
}

struct DeflateCtx {
    std::mutex mu;
    DevBuf match, crc, counts, z1k, dbg, off;
    DevBuf up, slots, packed;            // of bgzf_deflate_updown
    PinBuf h_counts, h_down;
    Event ev, t0, t1;
    int n_cu[64] = {0};
    int grid = 0;

    int open() {
        int dev = 0, rc;
        CTO_HIP(hipGetDevice(&dev));
        CTO_REQUIRE(dev >= 0 && dev < 64, CTO_EUNSUPPORTED, "cto_bgzf_deflate: device %d", dev);
        if (!n_cu[dev]) {
            int cus = 0;
            CTO_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
            CTO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_deflate), hipFuncAttributeMaxDynamicSharedMemorySize, int(kLdsBytes)));
            n_cu[dev] = std::max(1, cus);
        }
        grid = n_cu[dev];
        if (!ev.e) {
            uint32_t z[32];
            crc32_zero_1k_matrix(z);
            if ((rc = z1k.ensure(sizeof z)) || (rc = counts.ensure(64)) || (rc = h_counts.ensure(64)) || (rc = dbg.ensure(sizeof(DbgOut)))) return rc;
            CTO_HIP(hipMemcpy(z1k.p, z, sizeof z, hipMemcpyHostToDevice));
            if ((rc = t0.create()) || (rc = t1.create())) return rc;
            return ev.create(hipEventDisableTiming);
        }
        return CTO_OK;
    }
};
// the buffers of a context belong to one device: one context per device would be the next step; like the other entry points of the
// library the coder keeps one and is used from one device per process
DeflateCtx& ctx() { return process_wide<DeflateCtx>(); }

// queues CRC + coder under cx.mu; the counts are in cx.h_counts once the stream has been waited for
int queue_deflate(DeflateCtx& cx, const uint8_t* d_in, int64_t n, uint8_t* d_out, uint32_t* d_sizes, hipStream_t s, bool want_dbg) {
    const int64_t n_blocks = cdiv(n, df::kPayload);
    CTO_REQUIRE(n_blocks < (int64_t(1) << 30), CTO_EUNSUPPORTED, "cto_bgzf_deflate: more than 2^30 blocks in one call");
    int rc;
    if ((rc = cx.open())) return rc;
    const int grid = int(std::min<int64_t>(n_blocks, cx.grid));
    if ((rc = cx.match.ensure(size_t(grid) * df::kPayload * 4)) || (rc = cx.crc.ensure(size_t(n_blocks) * 4))) return rc;
    CTO_HIP(hipMemsetAsync(cx.counts.p, 0, 64, s));
    CTO_HIP(hipEventRecord(cx.t0, s));
    hipLaunchKernelGGL(k_crc32_values, dim3(unsigned(std::min<int64_t>(n_blocks, 4096))), dim3(64), 0, s, d_in, n, df::kPayload, int(n_blocks),
                       cx.z1k.as<uint32_t>(), cx.crc.as<uint32_t>());
    hipLaunchKernelGGL(k_deflate, dim3(unsigned(grid)), dim3(256), kLdsBytes, s, d_in, n, int(n_blocks), cx.crc.as<uint32_t>(), cx.match.as<uint32_t>(),
                       d_out, d_sizes, cx.counts.as<unsigned long long>(), want_dbg ? cx.dbg.as<DbgOut>() : nullptr);
    CTO_HIP(hipGetLastError());
    CTO_HIP(hipEventRecord(cx.t1, s));
    CTO_HIP(hipMemcpyAsync(cx.h_counts.p, cx.counts.p, 64, hipMemcpyDeviceToHost, s));
    return CTO_OK;
}

void add_counts(DeflateCtx& cx, int64_t n, cto_deflate_stats* st) {
    if (!st) return;
    const unsigned long long* c = cx.h_counts.as<unsigned long long>();
    float ms = 0;
    (void)hipEventElapsedTime(&ms, cx.t0, cx.t1);
    st->n_blocks += cdiv(n, df::kPayload);
    st->in_bytes += n;
    st->stored += int64_t(c[0]);
    st->fixed += int64_t(c[1]);
    st->dynamic += int64_t(c[2]);
    st->out_bytes += int64_t(c[3]);
    st->ms_kernels += double(ms);
}

}  // namespace

namespace cto {

int bgzf_deflate_device(const uint8_t* d_in, int64_t n, uint8_t* d_out, uint32_t* d_sizes, hipStream_t s, cto_deflate_stats* st) {
    if (n == 0) return CTO_OK;
    DeflateCtx& cx = ctx();
    std::lock_guard<std::mutex> lock(cx.mu);
    int rc;
    if ((rc = queue_deflate(cx, d_in, n, d_out, d_sizes, s, false))) return rc;
    CTO_HIP(record_and_wait(cx.ev, s));
    add_counts(cx, n, st);
    return CTO_OK;
}

int bgzf_deflate_host(const uint8_t* in, int64_t n, int threads, uint8_t* out, uint32_t* sizes, cto_deflate_stats* st) {
    const int64_t n_blocks = cdiv(n, df::kPayload);
    std::vector<int> types(size_t(n_blocks), 0);
    std::atomic<int64_t> next{0};
    auto work = [&] {
        df::BlockInfo info;
        for (int64_t b; (b = next.fetch_add(1)) < n_blocks;) {
            const int64_t at = b * df::kPayload;
            sizes[b] = uint32_t(df::encode_block(in + at, int(std::min<int64_t>(df::kPayload, n - at)), out + b * df::kSlot, &info));
            types[size_t(b)] = info.type;
        }
    };
    const int nt = int(std::min<int64_t>(std::max(1, std::min(threads, 64)), std::max<int64_t>(n_blocks, 1)));
    if (nt <= 1) work();
    else {
        std::vector<std::thread> th;
        for (int t = 0; t < nt; ++t) th.emplace_back(work);
        for (auto& x : th) x.join();
    }
    if (st) {
        st->n_blocks += n_blocks;
        st->in_bytes += n;
        for (int64_t b = 0; b < n_blocks; ++b) {
            st->out_bytes += sizes[b];
            ++(types[size_t(b)] == 0 ? st->stored : types[size_t(b)] == 1 ? st->fixed : st->dynamic);
        }
    }
    return CTO_OK;
}

namespace {
int down_locked(DeflateCtx& cx, const uint8_t* d_in, int64_t n, hipStream_t s, DevBuf* d_slots, DevBuf* d_packed, PinBuf* h_down, const uint32_t** sizes,
                const uint8_t** bytes, int64_t* n_bytes, cto_deflate_stats* st, double* ms_copy) {
    const int64_t n_blocks = cdiv(n, df::kPayload);
    const size_t head = align16(size_t(n_blocks) * 4);
    int rc;
    // packed: sizes | blocks, so that one copy brings both down
    if ((rc = d_slots->ensure(size_t(n_blocks) * df::kSlot)) || (rc = d_packed->ensure(head + size_t(n_blocks) * df::kSlot)) ||
        (rc = cx.off.ensure(size_t(n_blocks + 1) * 8)))
        return rc;
    uint32_t* d_sizes = d_packed->as<uint32_t>();
    if ((rc = queue_deflate(cx, d_in, n, d_slots->as<uint8_t>(), d_sizes, s, false))) return rc;
    hipLaunchKernelGGL(k_pack_offsets, dim3(1), dim3(64), 0, s, d_sizes, int(n_blocks), cx.off.as<unsigned long long>());
    hipLaunchKernelGGL(k_pack_copy, dim3(unsigned(n_blocks)), dim3(256), 0, s, d_slots->as<uint8_t>(), d_sizes, cx.off.as<unsigned long long>(),
                       d_packed->as<uint8_t>() + head);
    CTO_HIP(hipGetLastError());
    CTO_HIP(record_and_wait(cx.ev, s));                    // the counts: how many bytes to fetch
    add_counts(cx, n, st);
    const size_t total = size_t(cx.h_counts.as<unsigned long long>()[3]);
    CTO_REQUIRE(total <= size_t(n_blocks) * df::kSlot, CTO_EINVAL, "cto_bgzf_deflate: %zu bytes in %lld blocks", total, (long long)n_blocks);
    if ((rc = h_down->ensure(head + total))) return rc;
    CTO_HIP(hipEventRecord(cx.t0, s));
    CTO_HIP(hipMemcpyAsync(h_down->p, d_packed->p, head + total, hipMemcpyDeviceToHost, s));
    CTO_HIP(hipEventRecord(cx.t1, s));
    CTO_HIP(record_and_wait(cx.ev, s));
    if (ms_copy) { float ms = 0; (void)hipEventElapsedTime(&ms, cx.t0, cx.t1); *ms_copy += double(ms); }
    *sizes = h_down->as<uint32_t>();
    *bytes = h_down->as<uint8_t>() + head;
    *n_bytes = int64_t(total);
    return CTO_OK;
}
}  // namespace

int bgzf_deflate_down(const uint8_t* d_in, int64_t n, hipStream_t s, DevBuf* d_slots, DevBuf* d_packed, PinBuf* h_down, const uint32_t** sizes,
                      const uint8_t** bytes, int64_t* n_bytes, cto_deflate_stats* st, double* ms_copy) {
    *n_bytes = 0;
    *sizes = nullptr;
    *bytes = nullptr;
    if (n == 0) return CTO_OK;
    DeflateCtx& cx = ctx();
    std::lock_guard<std::mutex> lock(cx.mu);
    return down_locked(cx, d_in, n, s, d_slots, d_packed, h_down, sizes, bytes, n_bytes, st, ms_copy);
}

int bgzf_deflate_updown(const uint8_t* h_in, int64_t n, hipStream_t s, std::vector<uint8_t>* bytes, std::vector<uint32_t>* sizes, cto_deflate_stats* st) {
    bytes->clear();
    sizes->clear();
    if (n == 0) return CTO_OK;
    DeflateCtx& cx = ctx();
    std::lock_guard<std::mutex> lock(cx.mu);
    int rc;
    if ((rc = cx.up.ensure(size_t(n)))) return rc;
    CTO_HIP(hipMemcpyAsync(cx.up.p, h_in, size_t(n), hipMemcpyHostToDevice, s));
    const uint32_t* sz = nullptr;
    const uint8_t* by = nullptr;
    int64_t total = 0;
    if ((rc = down_locked(cx, cx.up.as<uint8_t>(), n, s, &cx.slots, &cx.packed, &cx.h_down, &sz, &by, &total, st, nullptr))) return rc;
    sizes->assign(sz, sz + cdiv(n, df::kPayload));
    bytes->assign(by, by + total);
    return CTO_OK;
}

}  // namespace cto

extern "C" int cto_bgzf_deflate(const void* in, int64_t n, int where, int host_threads, void* out, uint32_t* sizes, void* stream,
                                cto_deflate_stats* stats) {
    return guarded("cto_bgzf_deflate", [&]() -> int {
        CTO_REQUIRE(n >= 0 && (n == 0 || (in && out && sizes)), CTO_EINVAL, "cto_bgzf_deflate: null argument");
        CTO_REQUIRE(where == 0 || where == 1, CTO_EINVAL, "cto_bgzf_deflate: where must be 0 (device) or 1 (host)");
        cto_deflate_stats st{};
        int rc;
        if (where == 0) rc = bgzf_deflate_device(static_cast<const uint8_t*>(in), n, static_cast<uint8_t*>(out), sizes, static_cast<hipStream_t>(stream), &st);
        else {
            const int threads = host_threads > 0 ? host_threads : int(std::max(1u, std::min(std::thread::hardware_concurrency(), 16u)));
            rc = bgzf_deflate_host(static_cast<const uint8_t*>(in), n, threads, static_cast<uint8_t*>(out), sizes, &st);
        }
        if (stats) *stats = st;
        return rc;
    });
}

extern "C" int cto_deflate_code_lengths(const uint32_t* freq, int n_sym, int max_bits, int where, uint8_t* len) {
    return guarded("cto_deflate_code_lengths", [&]() -> int {
        CTO_REQUIRE(freq && len, CTO_EINVAL, "cto_deflate_code_lengths: null argument");
        CTO_REQUIRE(n_sym >= 2 && n_sym <= 288 && max_bits >= 1 && max_bits <= 15 && (int64_t(1) << max_bits) >= n_sym, CTO_EINVAL,
                    "cto_deflate_code_lengths: 2 .. 288 symbols, 1 .. 15 bits, 2^bits >= symbols");
        CTO_REQUIRE(where == 0 || where == 1, CTO_EINVAL, "cto_deflate_code_lengths: where must be 0 (device) or 1 (host)");
        uint64_t sum = 0;
        for (int i = 0; i < n_sym; ++i) sum += freq[i];
        CTO_REQUIRE(sum < (uint64_t(1) << 31), CTO_EINVAL, "cto_deflate_code_lengths: the frequencies sum to 2^31 or more");
        if (where == 1) {
            df::HuffWs ws;
            for (int s = 0; s < 288; ++s) ws.f_ll[s] = s < n_sym ? freq[s] : 0;
            df::force_pair(ws.f_ll, n_sym);
            df::sort_order(ws.f_ll, n_sym, ws.ord_ll);
            df::build_lengths(ws.f_ll, n_sym, ws.ord_ll, max_bits, &ws, len);
            return CTO_OK;
        }
        DevBuf d;
        int rc;
        if ((rc = d.ensure(288 * 4 + 288))) return rc;
        CTO_HIP(hipMemcpy(d.p, freq, size_t(n_sym) * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_code_lengths, dim3(1), dim3(256), 0, nullptr, d.as<uint32_t>(), n_sym, max_bits, d.as<uint8_t>() + 288 * 4);
        CTO_HIP(hipGetLastError());
        CTO_HIP(hipMemcpy(len, d.as<uint8_t>() + 288 * 4, size_t(n_sym), hipMemcpyDeviceToHost));
        return CTO_OK;
    });
}

extern "C" int cto_deflate_block_sizes(const uint8_t* block, int n, int where, int64_t bits[3], uint32_t hist[316]) {
    return guarded("cto_deflate_block_sizes", [&]() -> int {
        CTO_REQUIRE(n >= 0 && n <= df::kPayload && (block || n == 0) && bits && hist, CTO_EINVAL, "cto_deflate_block_sizes: 0 .. 0xff00 bytes");
        CTO_REQUIRE(where == 0 || where == 1, CTO_EINVAL, "cto_deflate_block_sizes: where must be 0 (device) or 1 (host)");
        if (where == 1 || n == 0) {
            std::vector<uint8_t> out(df::kSlot);
            df::BlockInfo info;
            df::encode_block(block, n, out.data(), &info);
            for (int k = 0; k < 3; ++k) bits[k] = info.bits[k];
            memcpy(hist, info.hist, sizeof info.hist);
            return CTO_OK;
        }
        DevBuf d_in, d_out;
        int rc;
        if ((rc = d_in.ensure(size_t(n))) || (rc = d_out.ensure(df::kSlot + 16))) return rc;
        CTO_HIP(hipMemcpy(d_in.p, block, size_t(n), hipMemcpyHostToDevice));
        DeflateCtx& cx = ctx();
        std::lock_guard<std::mutex> lock(cx.mu);
        if ((rc = queue_deflate(cx, d_in.as<uint8_t>(), n, d_out.as<uint8_t>() + 16, d_out.as<uint32_t>(), nullptr, true))) return rc;
        DbgOut h;
        CTO_HIP(hipMemcpy(&h, cx.dbg.p, sizeof h, hipMemcpyDeviceToHost));
        for (int k = 0; k < 3; ++k) bits[k] = h.bits[k];
        memcpy(hist, h.hist, sizeof h.hist);
        return CTO_OK;
    });
}
