// Alignment records on the device, shared by the front ends that read BAM there (pileup.hip: reads -> columns; allelecount.hip:
// per-locus allele counts): the inflated BGZF blocks of one chunk -> one contiguous record stream, every block checked against the
// CRC-32 of its gzip trailer, record boundaries from the offsets the .bai names, one DevRead per record.  RecordStream is the host
// driver that queues them.  File-local kernels: each source that includes this header gets its own copies.  (Host: bam_host.h.)
#pragma once
#include "bam_span.h"
#include "common.h"
#include "hip_buffers.h"
#include "scan.h"

namespace {

struct DevRead {
    uint32_t off;                 // of the record (its block_size field) in the linear stream
    int32_t pos, end;             // 0-based, end exclusive
    uint32_t ops_off;             // CIGAR operations (the field or the CG tag)
    int32_t n_ops;
    uint32_t seq_off, qual_off;
    int32_t l_seq;
    uint8_t mapq, rev, no_qual, valid;
};

struct Flags {                    // written by the kernels, read by the host after each phase
    int stop_idx, err_idx, paired_idx, skip_idx;    // first record index with the condition (INT_MAX: none)
    int bad_chain, deep_col, many_keys, ref_oob;
    int bad_crc;                                    // 1 + index of a block whose inflated bytes fail the gzip trailer's CRC-32 (0: none)
    int n_rec, n_valid, n_cols, n_keys;
    long long n_entries, key_str_bytes;
    int max_live, max_len;                          // largest number of accepted reads still open at another accepted read's start;
                                                    // longest reference span of an accepted read
};

__device__ __forceinline__ uint32_t ld16(const uint8_t* p) { return uint32_t(p[0]) | (uint32_t(p[1]) << 8); }
__device__ __forceinline__ uint32_t ld32(const uint8_t* p) { return uint32_t(p[0]) | (uint32_t(p[1]) << 8) | (uint32_t(p[2]) << 16) | (uint32_t(p[3]) << 24); }

__global__ void k_linearise(const uint8_t* __restrict__ src, const cto_bgzf_block* __restrict__ blocks, const int64_t* __restrict__ lin_off,
                            uint8_t* __restrict__ lin) {
    const cto_bgzf_block b = blocks[blockIdx.x];
    const uint8_t* s = src + b.out_off;
    uint8_t* d = lin + lin_off[blockIdx.x];
    for (uint32_t i = threadIdx.x; i < b.isize; i += blockDim.x) d[i] = s[i];
}

// CRC-32 of every inflated block against its gzip trailer, as htslib (and the host reader) checks it: one wave per block, lane k
// runs the byte-table CRC over its own slice (the first slice is the short one, every other one 1024 bytes), lane 0 then chains the
// 64 partial registers: state after slice k = P_k xor Z(state after slice k-1), Z = "1024 zero bytes" as a 32 x 32 bit matrix
// (z1k[i] = image of bit i, from the host) - a CRC register is linear in its start value.
struct CrcLds { uint32_t table[256], part[64], zm[32]; };
__device__ __forceinline__ void crc32_wave_setup(CrcLds& L, const uint32_t* __restrict__ z1k) {
    const int lane = threadIdx.x;
    for (int i = lane; i < 256; i += 64) {
        uint32_t c = uint32_t(i);
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
        L.table[i] = c;
    }
    if (lane < 32) L.zm[lane] = z1k[lane];
    __syncthreads();
}
// the CRC-32 of p[0 .. n), 0 < n <= 65536, by the one wave of the workgroup (every lane calls); lane 0 gets the value
__device__ __forceinline__ uint32_t crc32_wave(CrcLds& L, const uint8_t* __restrict__ p, int n) {
    const int lane = threadIdx.x;
    const int ns = (n + 1023) / 1024, r = n - 1024 * (ns - 1);
    uint32_t c = lane == 0 ? 0xFFFFFFFFu : 0u;
    if (lane < ns) {
        const int lo = lane == 0 ? 0 : r + 1024 * (lane - 1), len = lane == 0 ? r : 1024;
        for (int i = 0; i < len; ++i) c = L.table[(c ^ p[lo + i]) & 0xFFu] ^ (c >> 8);
    }
    __syncthreads();
    L.part[lane] = c;
    __syncthreads();
    uint32_t st = 0;
    if (lane == 0) {
        st = L.part[0];
        for (int k = 1; k < ns; ++k) {
            uint32_t z = 0;
            for (int i = 0; i < 32; ++i) z ^= ((st >> i) & 1u) ? L.zm[i] : 0u;
            st = L.part[k] ^ z;
        }
    }
    return st ^ 0xFFFFFFFFu;
}

__global__ __launch_bounds__(64) void k_crc32_blocks(const uint8_t* __restrict__ src, const cto_bgzf_block* __restrict__ blocks, int n_blocks,
                                                     const uint32_t* __restrict__ z1k, Flags* fl) {
    __shared__ CrcLds L;
    crc32_wave_setup(L, z1k);
    for (int b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const cto_bgzf_block bd = blocks[b];
        const int n = int(bd.isize);
        if (n == 0) continue;
        const uint32_t crc = crc32_wave(L, src + bd.out_off, n);
        if (threadIdx.x == 0 && crc != bd.crc32) atomicCAS(&fl->bad_crc, 0, b + 1);
    }
}

// the sibling for a writer: the CRC-32 of every `payload` bytes of src[0 .. n) (the last run shorter) to crc[b]
__global__ __launch_bounds__(64) void k_crc32_values(const uint8_t* __restrict__ src, int64_t n, int payload, int n_blocks,
                                                     const uint32_t* __restrict__ z1k, uint32_t* __restrict__ crc) {
    __shared__ CrcLds L;
    crc32_wave_setup(L, z1k);
    for (int b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const int64_t at = int64_t(b) * payload;
        const uint32_t v = crc32_wave(L, src + at, int(min(int64_t(payload), n - at)));
        if (threadIdx.x == 0) crc[b] = v;
    }
}

// chain k walks the records from starts[k] to starts[k + 1]; mode 0 counts, mode 1 writes their offsets at base[k]..
__global__ void k_chain(const uint8_t* __restrict__ lin, int64_t len, const int64_t* __restrict__ starts, int n_chains, int mode,
                        int* __restrict__ counts, const int* __restrict__ base, uint32_t* __restrict__ rec_off, Flags* fl) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_chains) return;
    int64_t o = starts[k];
    const int64_t limit = starts[k + 1];
    int n = 0;
    while (o < limit && o + 4 <= len) {
        const int64_t bsz = int64_t(int32_t(ld32(lin + o)));
        if (bsz < 32) { atomicExch(&fl->bad_chain, 2); break; }
        if (o + 4 + bsz > len) break;                         // the span ends inside a record the region does not need
        if (mode) rec_off[base[k] + n] = uint32_t(o);
        ++n;
        o += 4 + bsz;
    }
    if (o > limit) atomicExch(&fl->bad_chain, 1);              // a named offset that is not a record boundary
    if (!mode) counts[k] = n;
}

// The CIGAR of a record whose fixed fields hold up: the field itself, or the CG:B,I tag when the field is the long-CIGAR placeholder
// (<l_seq>S<ref_len>N); with it the reference and query bases the operations consume and whether one of them is an N.
struct DevCigar { const uint8_t* ops; int n_ops; long long rlen, qlen; bool has_skip; };
__device__ __forceinline__ DevCigar record_cigar(const uint8_t* b, int64_t bsz, const uint8_t* cg, int n_cig, const uint8_t* ql, int l_seq) {
    int n_ops = n_cig;
    const uint8_t* ops = cg;
    if (n_cig == 2 && (ld32(cg) & 15) == 4 && int(ld32(cg) >> 4) == l_seq && (ld32(cg + 4) & 15) == 3) {     // CG:B,I holds the real CIGAR
        const uint8_t* aux = ql + l_seq;
        const uint8_t* aend = b + bsz;
        while (aux + 3 <= aend) {
            const char t0 = char(aux[0]), t1 = char(aux[1]), ty = char(aux[2]);
            aux += 3;
            size_t skip = 0;
            if (ty == 'A' || ty == 'c' || ty == 'C') skip = 1;
            else if (ty == 's' || ty == 'S') skip = 2;
            else if (ty == 'i' || ty == 'I' || ty == 'f') skip = 4;
            else if (ty == 'Z' || ty == 'H') { while (aux + skip < aend && aux[skip]) ++skip; ++skip; }
            else if (ty == 'B') {
                if (aux + 5 > aend) break;
                const char sub = char(aux[0]);
                const uint32_t cnt = ld32(aux + 1);
                const size_t esz = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4;
                if (t0 == 'C' && t1 == 'G' && sub == 'I' && aux + 5 + size_t(cnt) * 4 <= aend) { n_ops = int(cnt); ops = aux + 5; break; }
                skip = 5 + size_t(cnt) * esz;
            } else break;
            aux += skip;
        }
    }
    long long rlen = 0, qlen = 0;
    bool has_skip = false;
    for (int k = 0; k < n_ops; ++k) {
        const uint32_t c = ld32(ops + size_t(k) * 4);
        const int opc = int(c & 15), len = int(c >> 4);
        if (opc == 0 || opc == 2 || opc == 3 || opc == 7 || opc == 8) rlen += len;
        if (opc == 0 || opc == 1 || opc == 4 || opc == 7 || opc == 8) qlen += len;
        has_skip |= opc == 3;
    }
    return DevCigar{ops, n_ops, rlen, qlen, has_skip};
}

// One lane per record: the fixed fields, the consumer's header filter accept(flag, mapq), the CIGAR's lengths, the region test; the
// first record that ends the region's scan lowers stop_idx.  PILEUP: a missing quality string and the first N operation are noted too.
template <bool PILEUP, class Accept>
__device__ __forceinline__ void parse_record(const uint8_t* __restrict__ lin, const uint32_t* __restrict__ rec_off, int n_rec, int tid, int beg0,
                                             int end0, Accept accept, DevRead* __restrict__ reads, Flags* fl) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rec) return;
    DevRead r{};
    r.off = rec_off[i];
    const uint8_t* b = lin + r.off + 4;
    const int64_t bsz = int64_t(int32_t(ld32(lin + r.off)));
    const int rtid = int(ld32(b)), pos = int(ld32(b + 4));
    const int l_name = b[8], mapq = b[9];
    const int n_cig = int(ld16(b + 12)), flag = int(ld16(b + 14));
    const int l_seq = int(ld32(b + 16));
    bool stop = false, ok = false;
    if (rtid != tid) stop = rtid > tid || rtid < 0;
    else if (pos >= end0) stop = true;
    else ok = accept(flag, mapq) && n_cig != 0 && l_seq > 0 && pos >= 0;
    if (stop) atomicMin(&fl->stop_idx, i);
    if (ok) {
        const int64_t need = 32 + int64_t(l_name) + int64_t(n_cig) * 4 + int64_t((l_seq + 1) / 2) + int64_t(l_seq);
        if (need > bsz) { atomicMin(&fl->err_idx, i); ok = false; }
    }
    if (ok) {
        const uint8_t* cg = b + 32 + l_name;
        const uint8_t* sq = cg + size_t(n_cig) * 4;
        const uint8_t* ql = sq + (l_seq + 1) / 2;
        const DevCigar dc = record_cigar(b, bsz, cg, n_cig, ql, l_seq);
        if (dc.qlen != l_seq || dc.rlen == 0) ok = false;
        else if (int64_t(pos) + dc.rlen > 0x7fffffffLL) { atomicMin(&fl->err_idx, i); ok = false; }
        else if (pos + dc.rlen <= beg0) ok = false;
        if (ok) {
            r.pos = pos;
            r.end = int32_t(pos + dc.rlen);
            r.ops_off = uint32_t(dc.ops - lin);
            r.n_ops = dc.n_ops;
            r.seq_off = uint32_t(sq - lin);
            r.qual_off = uint32_t(ql - lin);
            r.l_seq = l_seq;
            r.mapq = uint8_t(mapq);
            r.rev = (flag & 16) != 0;
            r.valid = 1;
            if (flag & 1) atomicMin(&fl->paired_idx, i);
            if (PILEUP) {
                r.no_qual = ql[0] == 0xff;
                if (dc.has_skip) atomicMin(&fl->skip_idx, i);
            }
        }
    }
    reads[i] = r;
}

// the column pile-up's filters: unmapped, excluded flags, MAPQ, orphans
__global__ void k_parse(const uint8_t* __restrict__ lin, const uint32_t* __restrict__ rec_off, int n_rec, int tid, int beg0, int end0,
                        int excl_flags, int min_mq, DevRead* __restrict__ reads, Flags* fl) {
    parse_record<true>(lin, rec_off, n_rec, tid, beg0, end0, [=](int flag, int mapq) {
        return !((flag & excl_flags) || (flag & 4) || mapq < min_mq || ((flag & 1) && !(flag & 2))); }, reads, fl);
}

// "1024 zero bytes" as a 32 x 32 bit matrix over CRC-32 registers (k_crc32_blocks chains the 64 lanes' partial registers with it)
inline void crc32_zero_1k_matrix(uint32_t z[32]) {
    uint32_t tbl[256];
    for (uint32_t i = 0; i < 256; ++i) { uint32_t c = i; for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1; tbl[i] = c; }
    for (int i = 0; i < 32; ++i) { uint32_t c = 1u << i; for (int k = 0; k < 1024; ++k) c = tbl[c & 0xFFu] ^ (c >> 8); z[i] = c; }
}

// The front half of a chunk on the device, from inflated blocks to record offsets: the buffers, the page-locked mirror of the flags
// and the event the waits sleep on (record_and_wait: hipStreamSynchronize polls the completion signal from the calling thread, and
// that thread shares the host's cores with everything else of a run).  One chunk at a time, everything on the caller's stream.
struct RecordStream {
    cto::DevBuf lin, counts, base, rec_off, z1k, up;
    cto::DevBuf tile_a, tile_tot;        // tile sums of the spread-out scans
    // The chunk's small inputs go up as ONE copy out of page-locked memory: separate hipMemcpyAsync calls from pageable vectors each
    // pin their source on the fly, under a lock every producer thread of a run shares.
    cto::PinBuf h_up, h_flags;
    cto::Event ev;
    cto::UploadParts parts;              // of the chunk's upload block
    Flags* fl = nullptr;                 // the chunk's flags on the device (its first part)
    const int64_t* d_starts = nullptr;
    int64_t len = 0;
    int n_chains = 0;

    int init() {                         // before the first wait; begin calls it too
        if (ev.e) return CTO_OK;
        uint32_t z[32];                  // "1024 zero bytes" as a bit matrix, once per context
        crc32_zero_1k_matrix(z);
        int rc;
        if ((rc = h_flags.ensure(sizeof(Flags))) || (rc = z1k.ensure(sizeof(z)))) return rc;
        CTO_HIP(hipMemcpy(z1k.p, z, sizeof(z), hipMemcpyHostToDevice));
        return ev.create(hipEventDisableTiming);          // last: its handle says that the rest is there
    }
    // scan.h's exclusive scan, its tile scratch grown to fit
    template <class Out> int scan(hipStream_t s, const int* in, int n, Out* out, Out* sum) {
        int rc;
        if ((rc = tile_a.ensure(size_t(cto::cdiv(n, SCAN_TILE) + 1) * 8)) || (rc = tile_tot.ensure(64))) return rc;
        scan_exclusive(s, in, n, out, sum, tile_a.as<long long>(), tile_tot.as<long long>());
        return CTO_OK;
    }
    int copy_flags(hipStream_t s) { CTO_HIP(hipMemcpyAsync(h_flags.p, fl, sizeof(Flags), hipMemcpyDeviceToHost, s)); return CTO_OK; }
    int wait(hipStream_t s) { CTO_HIP(cto::record_and_wait(ev, s)); return CTO_OK; }
    int fetch_flags(hipStream_t s) { const int rc = copy_flags(s); return rc != CTO_OK ? rc : wait(s); }
    void chain(hipStream_t s, int mode) {
        hipLaunchKernelGGL(k_chain, dim3(unsigned(cto::cdiv(n_chains, 64))), dim3(64), 0, s, lin.as<uint8_t>(), len, d_starts, n_chains, mode,
                           counts.as<int>(), mode ? base.as<int>() : nullptr, mode ? rec_off.as<uint32_t>() : nullptr, fl);
    }

    template <class T> T* extra(int i) const { return parts.at<T>(up.p, 4 + i); }       // the caller's i-th part on the device

    // One upload: flags | linear offsets | block table | record starts | the caller's `extra` parts.  Then CRC-32 of every block, the
    // linear stream, the records of every chain counted and the counts scanned; the flags come back behind one sleeping wait: h_flags
    // has bad_crc, bad_chain and n_rec for the caller to judge.
    // `t.n_chains` must be positive and `t.len` below 2^32 - 65536 (record offsets are 32-bit).
    int begin(hipStream_t s, const void* d_inflated, const cto_bgzf_block* h_blocks, int64_t n_blocks, const cto::SpanTables& t,
              const cto::UploadParts& extra) {
        int rc;
        len = t.len;
        n_chains = t.n_chains;
        if ((rc = init()) || (rc = lin.ensure(size_t(len) + 64)) || (rc = counts.ensure(size_t(n_chains + 1) * 4)) ||
            (rc = base.ensure(size_t(n_chains + 2) * 4)))
            return rc;
        Flags clean{};
        clean.stop_idx = clean.err_idx = clean.paired_idx = clean.skip_idx = 0x7fffffff;
        *h_flags.as<Flags>() = clean;
        parts = cto::UploadParts();
        parts.add(&clean, sizeof(Flags));
        parts.add(t.lin_off.data(), t.lin_off.size() * 8);
        parts.add(h_blocks, size_t(n_blocks) * sizeof(cto_bgzf_block));
        parts.add(t.starts.data(), t.starts.size() * 8);
        for (int i = 0; i < extra.n; ++i) parts.add(extra.src[i], extra.bytes[i]);
        if ((rc = up.ensure(parts.total)) || (rc = h_up.ensure(parts.total))) return rc;
        parts.stage(h_up.as<char>());
        CTO_HIP(hipMemcpyAsync(up.p, h_up.p, parts.total, hipMemcpyHostToDevice, s));
        fl = parts.at<Flags>(up.p, 0);
        const cto_bgzf_block* d_blocks = parts.at<cto_bgzf_block>(up.p, 2);
        d_starts = parts.at<int64_t>(up.p, 3);
        const uint8_t* src = static_cast<const uint8_t*>(d_inflated);
        hipLaunchKernelGGL(k_crc32_blocks, dim3(unsigned(std::min<int64_t>(n_blocks, 4096))), dim3(64), 0, s, src, d_blocks, int(n_blocks),
                           z1k.as<uint32_t>(), fl);
        hipLaunchKernelGGL(k_linearise, dim3(unsigned(n_blocks)), dim3(256), 0, s, src, d_blocks, parts.at<int64_t>(up.p, 1), lin.as<uint8_t>());
        chain(s, 0);
        if ((rc = scan(s, counts.as<int>(), n_chains, base.as<int>(), &fl->n_rec))) return rc;
        CTO_HIP(hipGetLastError());
        return fetch_flags(s);
    }
    // the offsets of the chunk's n_rec records, in file order, in rec_off
    int offsets(hipStream_t s, int n_rec) {
        const int rc = rec_off.ensure(size_t(n_rec) * 4);
        if (rc == CTO_OK) chain(s, 1);
        return rc;
    }
};

}  // namespace
