// Coverage of a BAM and the mix of a share of a normal BAM into a share of a tumour BAM: what src/gen_contaminated_bam.py of the
// reference starts five external processes for (`mosdepth -n -x` twice, `samtools view -s` twice, `samtools merge`, `samtools index`).
// cto_bam_coverage and cto_bam_mix are the C entry points; the host path (csrc/bam.cpp on bam_host.h) is the plain definition of the
// rules below and the device path in this file is held equal to it: tables equal, files byte for byte (tests/test_gpu_contam.py).
//
// PARITY UNPINNED against mosdepth and samtools: neither program exists on the build or GPU machines.  The rules are the definition;
// tests/test_gen_contaminated_bam.py holds them against a naive restatement (tests/contamutil.py).  All arithmetic is integer.
//
// Rules (positions 0-based):
//   a. coverage (`mosdepth -n -x`, its default filters).  For one contig of length L a record counts when its tid is the contig's,
//      pos >= 0 and flag & 1796 == 0; any MAPQ counts.  Its span is [pos, min(pos + rlen, L)), rlen the reference length of its CIGAR
//      (the CG:B,I tag when the field is the long-CIGAR placeholder: record_cigar).  Nothing inside the CIGAR is looked at and mates are
//      not de-overlapped; rlen == 0 counts nothing.  depth(p) = the number of spans that hold p; bases = the sum of depth(p); min and
//      max over p in [0, L); a contig without records has 0 / 0 / 0.  (Not parse_record: its l_seq > 0 and qlen == l_seq tests are the
//      pile-up's, not mosdepth's.)
//   b. keep (`samtools view -s SEED.ddd`).  For the read name's bytes b0 .. bn-1 (without the NUL, unsigned), all mod 2^32: h = b0,
//      h = h * 31 + bi for each further byte, 0 for the empty name; k = h ^ seed; k += ~(k << 15); k ^= k >> 10; k += k << 3;
//      k ^= k >> 6; k += ~(k << 11); k ^= k >> 16.  With the proportion as m thousandths the record is kept iff
//      (k & 0xffffff) * 1000 < m * 2^24 - the comparison of doubles that samtools makes, a tie being possible only where 125 divides m,
//      and those fractions are exact.  m == 1000 keeps everything, m == 0 nothing (samtools: -s 0.000 switches subsampling off and
//      keeps all - a deliberate difference).  Mates share a name, so pairs stay together.  No flag or MAPQ filter: every record whose
//      tid is the contig's and whose pos is not negative is a candidate; records without a reference are never copied.
//   c. merge.  Per contig the kept tumour records and the kept normal records form one sequence ordered by pos; equal pos: tumour
//      before normal; within one source: file order (samtools also orders equal positions by strand; this does not).  Output rank of
//      tumour record i: i + #{normal j : pos_j < pos_i}; of normal record j: j + #{tumour i : pos_i <= pos_j}.  A source whose positions
//      fall within a contig is an error ("not coordinate-sorted").  The header is the tumour's, verbatim; the normal's reference list
//      (count, names, lengths) must equal the tumour's.
//   d. output.  `BAM\1` + header + records in BGZF blocks of 0xff00 inflated bytes, zlib level 6 (stored when a block would not fit),
//      the empty end block; the .bai by the rules of phase_tumor.haplotag_bam: bins from the records' own bin field, adjacent chunks of
//      a bin joined, 16 kb linear index from pos and the CIGAR field's reference length, `0, 0` for contigs without written records.
//      The bytes depend neither on the number of threads nor on device versus host.
//
// Both calls walk a contig in position windows [w0, w1), runs of 16 kb index windows cut so that the inflated bytes of the span(s) stay
// under a budget (contam_plan_windows).  A window owns the records with w0 <= pos < w1: cto_bam_chunk_span also delivers records that
// start earlier - an earlier window's, dropped - and the first record with pos >= w1 stops the scan.  Windows are independent, so the
// merged output of a window is appended behind the one before it; of the coverage only the ends of the spans that reach past w1 go on
// to the next window.
//
// Device path, per window and source the shared front end (cto_bam_chunk_span, cto_bgzf_scan, copy up, cto_bgzf_inflate, RecordStream:
// CRC-32, linear stream, record chains), then
//   k_cov_parse    one lane per record: rule a - pos and clipped end, or the record marked out - and the stop test
//   k_cov_diff     one lane per counted record and per carried end: +1 at pos - w0, -1 at end - w0 when the span ends inside the window
//                  (integer atomics); bases through a workgroup reduction and one 64-bit atomic per workgroup; spans that reach past the
//                  window are marked, compacted and come down as a list of ends as long as the depth at the window's edge
//   scan.h's scan over the window, k_cov_minmax over its prefix sums
//   k_view_parse   one lane per record of a source: pos, byte length, candidate and keep bit (rule b; the hash is sequential over at
//                  most 254 bytes per lane - the records are resident and this is not the long pole), a flag where pos falls below
//                  the predecessor's
//   k_view_marks / scan / k_compact   the kept records of a source, compacted
//   k_merge_rank   one lane per kept record: one binary search in the other source's kept positions gives its rank (rule c); its
//                  length goes to that rank
//   scan of the lengths in rank order: every record's offset in the window's output stream
//   k_gather       one wave per kept record copies 4 + block_size bytes from its source's linear stream to its offset (records are not
//                  aligned and may be longer than 64 KB) and writes its index row: pos, rlen, bin, offset
// Only the merged stream and the rows come down; the host cuts header + stream into blocks, deflates them on host_threads threads, writes
// them in order and builds the .bai (MixWriter, csrc/bam.cpp).  A window that does not inflate, fails a CRC-32 or has a broken record
// chain is redone by the host path (stats.fallback_chunks).
#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "bam_records.h"
#include "common.h"
#include "deflate_internal.h"
#include "hip_buffers.h"
#include "inflated_span.h"
#include "pack_internal.h"
#include "scan.h"

using namespace cto;

namespace {

struct CovOut { unsigned long long bases; int mn, mx; };

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
    return v;                                                      // lane 0 holds the sum
}

// rule a, and the window's stop test
__global__ void k_cov_parse(const uint8_t* __restrict__ lin, const uint32_t* __restrict__ rec_off, int n_rec, int tid, int w0, int e1, int L,
                            int* __restrict__ cpos, int* __restrict__ cend, Flags* fl) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rec) return;
    const uint32_t off = rec_off[i];
    const uint8_t* b = lin + off + 4;
    const int64_t bsz = int64_t(int32_t(ld32(lin + off)));
    const int rtid = int(ld32(b)), pos = int(ld32(b + 4));
    const int l_name = b[8], n_cig = int(ld16(b + 12)), flag = int(ld16(b + 14)), l_seq = int(ld32(b + 16));
    bool stop = false, ok = false;
    if (rtid != tid) stop = rtid > tid || rtid < 0;
    else if (pos >= e1) stop = true;
    else ok = pos >= w0 && !(flag & kCovExclFlags);
    if (stop) atomicMin(&fl->stop_idx, i);
    int p = -1, e = -1;
    if (ok) {
        const int64_t ls = l_seq < 0 ? 0 : l_seq;
        const int64_t need = 32 + int64_t(l_name) + int64_t(n_cig) * 4 + (ls + 1) / 2 + ls;
        if (l_seq < 0 || need > bsz) atomicMin(&fl->err_idx, i);
        else {
            const uint8_t* cg = b + 32 + l_name;
            const uint8_t* ql = cg + size_t(n_cig) * 4 + (l_seq + 1) / 2;
            const DevCigar dc = record_cigar(b, bsz, cg, n_cig, ql, l_seq);
            const long long end = min((long long)pos + dc.rlen, (long long)L);
            if (end > pos) { p = pos; e = int(end); }
        }
    }
    cpos[i] = p;
    cend[i] = e;
}

__global__ __launch_bounds__(256) void k_cov_diff(const int* __restrict__ cpos, const int* __restrict__ cend, int n_rec, Flags* fl,
                                                  const int* __restrict__ carry, int n_carry, int w0, int e1, int* __restrict__ diff,
                                                  int* __restrict__ open, CovOut* out) {
    __shared__ long long wsum[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    long long add = 0;
    if (i < n_rec) {
        int o = 0;
        const int p = cpos[i], e = cend[i];
        if (i < fl->stop_idx && p >= w0 && p < e1 && e > p) {
            atomicAdd(&diff[p - w0], 1);
            if (e < e1) atomicAdd(&diff[e - w0], -1);
            add = min(e, e1) - p;
            o = e > e1;
            atomicAdd(&fl->n_cols, 1);                             // the records counted
        }
        open[i] = o;
    } else if (i < n_rec + n_carry) {
        const int e = carry[i - n_rec];
        if (e > w0) {
            if (e < e1) atomicAdd(&diff[e - w0], -1);
            add = min(e, e1) - w0;
        }
    }
    add = wave_sum(add);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = add;
    __syncthreads();
    if (threadIdx.x == 0) {
        const long long t = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (t) atomicAdd(&out->bases, (unsigned long long)t);
    }
}

__global__ void k_open_write(const int* __restrict__ open, const int* __restrict__ at, const int* __restrict__ cend, int n_rec,
                             int* __restrict__ ends) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_rec && open[i]) ends[at[i]] = cend[i];
}

// psum: the exclusive prefix sums of diff[0 .. n): psum[p + 1] = depth(w0 + p) - the depth the window starts at
__global__ __launch_bounds__(256) void k_cov_minmax(const int* __restrict__ psum, int n, CovOut* out) {
    int lo = INT_MAX, hi = INT_MIN;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < n; p += gridDim.x * 256) {
        const int d = psum[p + 1];
        lo = min(lo, d);
        hi = max(hi, d);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        lo = min(lo, __shfl_down(lo, d));
        hi = max(hi, __shfl_down(hi, d));
    }
    if ((threadIdx.x & 63) == 0 && lo <= hi) {
        atomicMin(&out->mn, lo);
        atomicMax(&out->mx, hi);
    }
}

// rule b on the device (the host's: subsample_key in pack_internal.h)
__device__ __forceinline__ uint32_t dev_subsample_key(const uint8_t* name, int n, uint32_t seed) {
    uint32_t h = n > 0 ? name[0] : 0;
    for (int i = 1; i < n; ++i) h = h * 31u + name[i];
    uint32_t k = h ^ seed;
    k += ~(k << 15); k ^= k >> 10; k += k << 3; k ^= k >> 6; k += ~(k << 11); k ^= k >> 16;
    return k & 0xffffffu;
}

// One lane per record of a source: bit 0 of ck = candidate, bit 1 = kept.  skip_idx takes the first record whose pos falls below its
// predecessor's, both being the contig's.
__global__ void k_view_parse(const uint8_t* __restrict__ lin, const uint32_t* __restrict__ rec_off, int n_rec, int tid, int w0, int w1,
                             uint32_t seed, int m, int* __restrict__ pos_out, int* __restrict__ len_out, uint8_t* __restrict__ ck, Flags* fl) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rec) return;
    const uint32_t off = rec_off[i];
    const uint8_t* b = lin + off + 4;
    const int64_t bsz = int64_t(int32_t(ld32(lin + off)));
    const int rtid = int(ld32(b)), pos = int(ld32(b + 4));
    const int l_name = b[8], n_cig = int(ld16(b + 12));
    bool stop = false, mine = false;
    if (rtid != tid) stop = rtid > tid || rtid < 0;
    else if (pos >= w1) stop = true;
    else mine = true;
    if (stop) atomicMin(&fl->stop_idx, i);
    uint8_t bits = 0;
    if (mine) {
        if (i > 0) {
            const uint8_t* pb = lin + rec_off[i - 1] + 4;
            if (int(ld32(pb)) == tid && pos < int(ld32(pb + 4))) atomicMin(&fl->skip_idx, i);
        }
        if (pos >= w0) {
            if (32 + int64_t(l_name) + int64_t(n_cig) * 4 > bsz) atomicMin(&fl->err_idx, i);
            else bits = 1 | (uint64_t(dev_subsample_key(b + 32, max(0, l_name - 1), seed)) * 1000u < (uint64_t(uint32_t(m)) << 24) ? 2 : 0);
        }
    }
    pos_out[i] = pos;
    len_out[i] = int(4 + bsz);
    ck[i] = bits;
}

__global__ void k_view_marks(const uint8_t* __restrict__ ck, int n_rec, Flags* fl, int* __restrict__ mark) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rec) return;
    const bool in = i < fl->stop_idx;
    mark[i] = in && (ck[i] & 2);
    if (in && (ck[i] & 1)) atomicAdd(&fl->n_cols, 1);              // the candidates
}

__global__ void k_compact(const int* __restrict__ mark, const int* __restrict__ at, const int* __restrict__ pos, int n_rec,
                          int* __restrict__ kpos, int* __restrict__ kidx) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_rec && mark[i]) { kpos[at[i]] = pos[i]; kidx[at[i]] = i; }
}

// what k_merge_rank and k_gather read of one source
struct KeptSrc { const uint8_t* lin; const uint32_t* rec_off; const int *len, *kpos, *kidx; int n; };

// rule c: kept record g of the two sources (the tumour's first) -> its rank; its length and where it comes from go there
__global__ void k_merge_rank(KeptSrc T, KeptSrc N, int* __restrict__ rlen, uint32_t* __restrict__ rsrc) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= T.n + N.n) return;
    const bool tumour = g < T.n;
    const int i = tumour ? g : g - T.n;
    const KeptSrc& me = tumour ? T : N;
    const KeptSrc& other = tumour ? N : T;
    const int p = me.kpos[i];
    int a = 0, b = other.n;                                        // tumour: the normal records with pos < p; normal: the tumour's with pos <= p
    while (a < b) {
        const int mid = (a + b) >> 1, q = other.kpos[mid];
        if (tumour ? q < p : q <= p) a = mid + 1; else b = mid;
    }
    const int rank = i + a, rec = me.kidx[i];
    rlen[rank] = me.len[rec];
    rsrc[rank] = (tumour ? 0u : 0x80000000u) | uint32_t(rec);
}

// One wave per output record: its bytes to roff[rank] of the window's stream, aligned words where the destination allows; its index row.
__global__ __launch_bounds__(256) void k_gather(KeptSrc T, KeptSrc N, const uint32_t* __restrict__ rsrc, const long long* __restrict__ roff,
                                                int n_out, uint8_t* __restrict__ out, MixRow* __restrict__ rows) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_out) return;
    const uint32_t sr = rsrc[r];
    const KeptSrc& S = (sr >> 31) ? N : T;
    const int rec = int(sr & 0x7fffffffu);
    const uint8_t* src = S.lin + S.rec_off[rec];
    const long long n = S.len[rec], dst0 = roff[r];
    uint8_t* dst = out + dst0;
    const long long head = min(n, (long long)((4 - (dst0 & 3)) & 3)), words = (n - head) >> 2;
    if (lane < head) dst[lane] = src[lane];
    uint32_t* dw = reinterpret_cast<uint32_t*>(dst + head);
    for (long long k = lane; k < words; k += 64) dw[k] = ld32(src + head + 4 * k);
    const long long tail = head + 4 * words;
    if (tail + lane < n) dst[tail + lane] = src[tail + lane];
    // the index row: the reference length of the CIGAR field, as phase_tumor.haplotag_bam takes it
    const uint8_t* b = src + 4;
    const int l_name = b[8], n_cig = int(ld16(b + 12));
    long long rl = 0;
    for (int k = lane; k < n_cig; k += 64) {
        const uint32_t c = ld32(b + 32 + l_name + size_t(k) * 4);
        const int opc = int(c & 15);
        if (opc == 0 || opc == 2 || opc == 3 || opc == 7 || opc == 8) rl += c >> 4;
    }
    rl = wave_sum(rl);
    if (lane == 0) rows[r] = MixRow{int(ld32(b + 4)), int(min(rl, (long long)INT_MAX)), int(ld16(b + 10)), 0, dst0};
}

enum { CHUNK_DONE = 0, CHUNK_DAMAGED = 1, CHUNK_NOTHING = 2, CHUNK_TOO_LARGE = 3 };

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
float elapsed(hipEvent_t a, hipEvent_t b) { float ms = 0.f; (void)hipEventElapsedTime(&ms, a, b); return ms; }

// One source of one window on its way to record offsets
struct Source {
    InflatedSpan span;
    RecordStream rs;
    SpanTables tables;
    DevBuf pos, len, ck, mark, at, kpos, kidx;
    int64_t n_blocks = 0;
    int32_t tid = -1;
    int n_rec = 0, n_kept = 0;
    bool empty = true;                   // the index names nothing for the window

    // file range, bytes and block table, record starts: everything before the device; *outcome CHUNK_DONE also for an empty source
    int read(const char* who, const char* bam_path, const char* bai_path, const char* ctg_name, int64_t w0, int64_t w1, int* outcome) {
        *outcome = CHUNK_DONE;
        empty = true;
        n_rec = n_kept = 0;
        int64_t fb = 0, fe = 0;
        int rc = cto_bam_chunk_span(bam_path, bai_path, ctg_name, w0 + 1, w1, &fb, &fe);
        if (rc != CTO_OK) return rc;
        if (fe <= fb) return CTO_OK;
        if ((rc = span.read(bam_path, fb, size_t(fe - fb), who))) return rc;
        n_blocks = span.scan();
        if (n_blocks == CTO_EINVAL) { *outcome = CHUNK_DAMAGED; return CTO_OK; }
        if (n_blocks < 0) return int(n_blocks);
        if (n_blocks == 0) return CTO_OK;
        tables.lay_out(span.blocks(), n_blocks);
        if (tables.len >= (int64_t(1) << 32) - 65536 || n_blocks >= (int64_t(1) << 30)) { *outcome = CHUNK_TOO_LARGE; return CTO_OK; }
        std::vector<uint64_t> voffs;
        const int64_t n_st = record_starts(bam_path, bai_path, ctg_name, w0 + 1, w1, fb, fe, &voffs, &tid);
        if (n_st < 0) return int(n_st);
        tables.map_starts(span.blocks(), n_blocks, voffs.data(), n_st);
        empty = tables.n_chains == 0;
        return CTO_OK;
    }
    // CRC-32, linear stream, record chains and offsets behind the inflate; *outcome CHUNK_DAMAGED when one of them fails
    int records(hipStream_t s, const UploadParts& extra, cto_contam_stats* st, int* outcome) {
        int rc;
        if ((rc = rs.begin(s, span.d_out.p, span.blocks(), n_blocks, tables, extra))) return rc;
        const Flags* hf = rs.h_flags.as<Flags>();
        st->n_blocks += n_blocks;
        st->inflated_bytes += tables.len;
        if (span.first_bad_status() >= 0 || hf->bad_crc || hf->bad_chain) { *outcome = CHUNK_DAMAGED; return CTO_OK; }
        n_rec = std::max(hf->n_rec, 0);
        if (n_rec == 0) { empty = true; return CTO_OK; }
        return rs.offsets(s, n_rec);
    }
};

struct ContamCtx {
    std::mutex mu;                                                  // one device call at a time: the buffers outlive the calls
    Source src[2];
    DevBuf cpos, cend, open, diff, psum, ends;                      // coverage
    DevBuf rlen, rsrc, roff, out, rows;                             // mix
    DevBuf d_slots, d_packed;                                       // mix with the device coder: its blocks in slots, back to back
    PinBuf h_cov, h_out, h_rows, h_coded;
    Event t[5];
};

// Rule a over the window [w0, w1) on the device; `carry` as cov_window_host takes and leaves it
int cov_window_device(ContamCtx* cx, const char* bam_path, const char* bai_path, const char* ctg_name, int64_t w0, int64_t w1, int64_t L,
                      std::vector<int32_t>* carry, hipStream_t s, cto_contam_stats* st, int64_t* bases, int32_t* mn, int32_t* mx, int* outcome) {
    const int64_t e1 = std::min(w1, L), n = e1 - w0;
    Source& S = cx->src[0];
    int rc;
    if ((rc = S.read("cto_bam_coverage: ", bam_path, bai_path, ctg_name, w0, e1, outcome)) || *outcome != CHUNK_DONE) return rc;
    if (S.empty) { *outcome = CHUNK_NOTHING; return CTO_OK; }
    const int n_carry = int(carry->size());
    const CovOut clean{0ull, INT_MAX, INT_MIN};
    UploadParts extra;
    extra.add(carry->data(), size_t(n_carry) * 4);
    extra.add(&clean, sizeof clean);
    CTO_HIP(hipEventRecord(cx->t[0], s));
    if ((rc = S.span.inflate(s))) return rc;
    CTO_HIP(hipEventRecord(cx->t[1], s));
    if ((rc = S.records(s, extra, st, outcome)) || *outcome != CHUNK_DONE) return rc;
    if (S.empty) { *outcome = CHUNK_NOTHING; return CTO_OK; }
    const int n_rec = S.n_rec;
    RecordStream& rs = S.rs;
    Flags* const fl = rs.fl;
    const Flags* hf = rs.h_flags.as<Flags>();
    if ((rc = cx->cpos.ensure(size_t(n_rec) * 4)) || (rc = cx->cend.ensure(size_t(n_rec) * 4)) || (rc = cx->open.ensure(size_t(n_rec) * 4)) ||
        (rc = S.at.ensure(size_t(n_rec + 1) * 4)) || (rc = cx->ends.ensure(size_t(n_rec) * 4)) || (rc = cx->diff.ensure(size_t(n + 1) * 4)) ||
        (rc = cx->psum.ensure(size_t(n + 2) * 4)) || (rc = cx->h_cov.ensure(sizeof(CovOut) + size_t(n_rec) * 4)))
        return rc;
    const int* d_carry = rs.extra<int>(0);
    CovOut* d_out = rs.extra<CovOut>(1);
    const unsigned rgrid = unsigned(cdiv(n_rec, 128));
    CTO_HIP(hipMemsetAsync(cx->diff.p, 0, size_t(n + 1) * 4, s));
    hipLaunchKernelGGL(k_cov_parse, dim3(rgrid), dim3(128), 0, s, rs.lin.as<uint8_t>(), rs.rec_off.as<uint32_t>(), n_rec, S.tid, int(w0), int(e1),
                       int(std::min<int64_t>(L, INT_MAX)), cx->cpos.as<int>(), cx->cend.as<int>(), fl);
    hipLaunchKernelGGL(k_cov_diff, dim3(unsigned(cdiv(int64_t(n_rec) + n_carry, 256))), dim3(256), 0, s, cx->cpos.as<int>(), cx->cend.as<int>(), n_rec,
                       fl, d_carry, n_carry, int(w0), int(e1), cx->diff.as<int>(), cx->open.as<int>(), d_out);
    if ((rc = rs.scan(s, cx->open.as<int>(), n_rec, S.at.as<int>(), &fl->n_valid))) return rc;
    hipLaunchKernelGGL(k_open_write, dim3(rgrid), dim3(128), 0, s, cx->open.as<int>(), S.at.as<int>(), cx->cend.as<int>(), n_rec, cx->ends.as<int>());
    if ((rc = rs.scan(s, cx->diff.as<int>(), int(n), cx->psum.as<int>(), static_cast<int*>(nullptr)))) return rc;
    hipLaunchKernelGGL(k_cov_minmax, dim3(unsigned(std::min<int64_t>(cdiv(n, 256), 2048))), dim3(256), 0, s, cx->psum.as<int>(), int(n), d_out);
    CTO_HIP(hipGetLastError());
    CTO_HIP(hipEventRecord(cx->t[2], s));
    if ((rc = rs.fetch_flags(s))) return rc;
    if (hf->err_idx < hf->stop_idx) { *outcome = CHUNK_DAMAGED; return CTO_OK; }
    const int n_open = hf->n_valid;
    CTO_HIP(hipMemcpyAsync(cx->h_cov.p, d_out, sizeof(CovOut), hipMemcpyDeviceToHost, s));
    if (n_open > 0) CTO_HIP(hipMemcpyAsync(cx->h_cov.as<char>() + sizeof(CovOut), cx->ends.p, size_t(n_open) * 4, hipMemcpyDeviceToHost, s));
    CTO_HIP(hipEventRecord(cx->t[3], s));
    if ((rc = rs.wait(s))) return rc;
    const CovOut* co = cx->h_cov.as<CovOut>();
    const int32_t* ends = reinterpret_cast<const int32_t*>(cx->h_cov.as<char>() + sizeof(CovOut));
    std::vector<int32_t> open;
    for (int32_t e : *carry) if (e > e1) open.push_back(e);
    open.insert(open.end(), ends, ends + n_open);
    *bases = int64_t(co->bases);
    *mn = co->mn + n_carry;
    *mx = co->mx + n_carry;
    carry->swap(open);
    st->n_records += hf->n_cols;
    st->ms_inflate += elapsed(cx->t[0], cx->t[1]);
    st->ms_kernels += elapsed(cx->t[1], cx->t[2]);
    st->ms_copy += elapsed(cx->t[2], cx->t[3]);
    return CTO_OK;
}

// Rules b and c over the window [w0, w1) on the device: the merged stream and its rows in cx->h_out / cx->h_rows
// carry (deflate on the device, else null): the bytes the writer holds behind its last block go up in front of the merged stream, the
// whole blocks of both are coded here (csrc/deflate.hip) and come down in *coded; the bytes behind them are in cx->h_out
struct CodedDown { const uint32_t* sizes = nullptr; const uint8_t* blocks = nullptr; int64_t n_blocks = 0, n_rest = 0; };
int mix_window_device(ContamCtx* cx, const char* const* bams, const char* const* bais, const char* ctg_name, int64_t w0, int64_t w1, const int* m,
                      uint32_t seed, hipStream_t s, cto_contam_stats* st, int64_t* n_bytes, int64_t* n_rows, MixCounts* counts, int* outcome,
                      const std::vector<uint8_t>* carry = nullptr, CodedDown* coded = nullptr, cto_deflate_stats* dst = nullptr) {
    *n_bytes = *n_rows = 0;
    *counts = MixCounts{};
    int rc;
    for (int k = 0; k < 2; ++k)
        if ((rc = cx->src[k].read("cto_bam_mix: ", bams[k], bais[k], ctg_name, w0, w1, outcome)) || *outcome != CHUNK_DONE) return rc;
    if (cx->src[0].empty && cx->src[1].empty) { *outcome = CHUNK_NOTHING; return CTO_OK; }
    CTO_HIP(hipEventRecord(cx->t[0], s));
    for (int k = 0; k < 2; ++k)
        if (!cx->src[k].empty && (rc = cx->src[k].span.inflate(s))) return rc;
    CTO_HIP(hipEventRecord(cx->t[1], s));
    for (int k = 0; k < 2; ++k) {
        Source& S = cx->src[k];
        if (S.empty) continue;
        if ((rc = S.records(s, UploadParts(), st, outcome)) || *outcome != CHUNK_DONE) return rc;
        if (S.empty) continue;
        const int n_rec = S.n_rec;
        if ((rc = S.pos.ensure(size_t(n_rec) * 4)) || (rc = S.len.ensure(size_t(n_rec) * 4)) || (rc = S.ck.ensure(size_t(n_rec))) ||
            (rc = S.mark.ensure(size_t(n_rec) * 4)) || (rc = S.at.ensure(size_t(n_rec + 1) * 4)) || (rc = S.kpos.ensure(size_t(n_rec) * 4)) ||
            (rc = S.kidx.ensure(size_t(n_rec) * 4)))
            return rc;
        const unsigned rgrid = unsigned(cdiv(n_rec, 128));
        Flags* const fl = S.rs.fl;
        hipLaunchKernelGGL(k_view_parse, dim3(rgrid), dim3(128), 0, s, S.rs.lin.as<uint8_t>(), S.rs.rec_off.as<uint32_t>(), n_rec, S.tid, int(w0),
                           int(std::min<int64_t>(w1, INT_MAX)), seed, m[k], S.pos.as<int>(), S.len.as<int>(), S.ck.as<uint8_t>(), fl);
        hipLaunchKernelGGL(k_view_marks, dim3(rgrid), dim3(128), 0, s, S.ck.as<uint8_t>(), n_rec, fl, S.mark.as<int>());
        if ((rc = S.rs.scan(s, S.mark.as<int>(), n_rec, S.at.as<int>(), &fl->n_valid))) return rc;
        hipLaunchKernelGGL(k_compact, dim3(rgrid), dim3(128), 0, s, S.mark.as<int>(), S.at.as<int>(), S.pos.as<int>(), n_rec, S.kpos.as<int>(),
                           S.kidx.as<int>());
        CTO_HIP(hipGetLastError());
        if ((rc = S.rs.fetch_flags(s))) return rc;
        const Flags* hf = S.rs.h_flags.as<Flags>();
        // a record shorter than its fields, or positions that fall: the host path says which
        if (hf->err_idx < hf->stop_idx || hf->skip_idx < hf->stop_idx) { *outcome = CHUNK_DAMAGED; return CTO_OK; }
        S.n_kept = hf->n_valid;
        counts->cand[k] = hf->n_cols;
        counts->kept[k] = hf->n_valid;
    }
    KeptSrc ks[2];
    for (int k = 0; k < 2; ++k) {
        const Source& S = cx->src[k];
        ks[k] = KeptSrc{S.rs.lin.as<uint8_t>(), S.rs.rec_off.as<uint32_t>(), S.len.as<int>(), S.kpos.as<int>(), S.kidx.as<int>(), S.empty ? 0 : S.n_kept};
    }
    const int64_t n_out = int64_t(ks[0].n) + ks[1].n;
    if (n_out == 0) { st->ms_inflate += elapsed(cx->t[0], cx->t[1]); return CTO_OK; }
    CTO_REQUIRE(n_out < (int64_t(1) << 31), CTO_EUNSUPPORTED, "cto_bam_mix: more than 2^31 records in one window");
    const Source& lead = cx->src[0].empty ? cx->src[1] : cx->src[0];             // whose stream's scratch and flags the merge uses
    RecordStream& rs = const_cast<RecordStream&>(lead.rs);
    int64_t room = 0;
    for (int k = 0; k < 2; ++k) if (!cx->src[k].empty) room += cx->src[k].tables.len;
    // the stream starts at a multiple of 4 (k_gather), the carried bytes end there
    const size_t n_carry = carry ? carry->size() : 0, slack = (4 - (n_carry & 3)) & 3;
    if ((rc = cx->rlen.ensure(size_t(n_out) * 4)) || (rc = cx->rsrc.ensure(size_t(n_out) * 4)) || (rc = cx->roff.ensure(size_t(n_out + 1) * 8)) ||
        (rc = cx->out.ensure(slack + n_carry + size_t(room) + 64)) || (rc = cx->rows.ensure(size_t(n_out) * sizeof(MixRow))))
        return rc;
    uint8_t* const d_stream = cx->out.as<uint8_t>() + slack + n_carry;
    if (n_carry) CTO_HIP(hipMemcpyAsync(cx->out.as<uint8_t>() + slack, carry->data(), n_carry, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_merge_rank, dim3(unsigned(cdiv(n_out, 128))), dim3(128), 0, s, ks[0], ks[1], cx->rlen.as<int>(), cx->rsrc.as<uint32_t>());
    if ((rc = rs.scan(s, cx->rlen.as<int>(), int(n_out), cx->roff.as<long long>(), &rs.fl->n_entries))) return rc;
    hipLaunchKernelGGL(k_gather, dim3(unsigned(cdiv(n_out, 4))), dim3(256), 0, s, ks[0], ks[1], cx->rsrc.as<uint32_t>(), cx->roff.as<long long>(),
                       int(n_out), d_stream, cx->rows.as<MixRow>());
    CTO_HIP(hipGetLastError());
    CTO_HIP(hipEventRecord(cx->t[2], s));
    if ((rc = rs.fetch_flags(s))) return rc;
    const int64_t total = rs.h_flags.as<Flags>()->n_entries;
    CTO_REQUIRE(total >= 0 && total <= room, CTO_EINVAL, "cto_bam_mix: the merged window has %lld bytes, its sources %lld", (long long)total,
                (long long)room);
    if (coded) {
        const int64_t all = int64_t(n_carry) + total, whole = all / CTO_BGZF_PAYLOAD * CTO_BGZF_PAYLOAD;
        const uint8_t* d_in = cx->out.as<uint8_t>() + slack;
        int64_t n_coded = 0;
        double ms_down = 0;
        if ((rc = bgzf_deflate_down(d_in, whole, s, &cx->d_slots, &cx->d_packed, &cx->h_coded, &coded->sizes, &coded->blocks, &n_coded, dst, &ms_down)))
            return rc;
        coded->n_blocks = whole / CTO_BGZF_PAYLOAD;
        coded->n_rest = all - whole;
        if ((rc = cx->h_out.ensure(size_t(coded->n_rest) + 64)) || (rc = cx->h_rows.ensure(size_t(n_out) * sizeof(MixRow)))) return rc;
        CTO_HIP(hipEventRecord(cx->t[3], s));
        if (coded->n_rest) CTO_HIP(hipMemcpyAsync(cx->h_out.p, d_in + whole, size_t(coded->n_rest), hipMemcpyDeviceToHost, s));
        CTO_HIP(hipMemcpyAsync(cx->h_rows.p, cx->rows.p, size_t(n_out) * sizeof(MixRow), hipMemcpyDeviceToHost, s));
        CTO_HIP(hipEventRecord(cx->t[4], s));
        if ((rc = rs.wait(s))) return rc;
        *n_bytes = total;
        *n_rows = n_out;
        st->ms_inflate += elapsed(cx->t[0], cx->t[1]);
        st->ms_kernels += elapsed(cx->t[1], cx->t[2]);
        st->ms_copy += ms_down + elapsed(cx->t[3], cx->t[4]);
        return CTO_OK;
    }
    if ((rc = cx->h_out.ensure(size_t(total) + 64)) || (rc = cx->h_rows.ensure(size_t(n_out) * sizeof(MixRow)))) return rc;
    CTO_HIP(hipEventRecord(cx->t[3], s));
    CTO_HIP(hipMemcpyAsync(cx->h_out.p, d_stream, size_t(total), hipMemcpyDeviceToHost, s));
    CTO_HIP(hipMemcpyAsync(cx->h_rows.p, cx->rows.p, size_t(n_out) * sizeof(MixRow), hipMemcpyDeviceToHost, s));
    CTO_HIP(hipEventRecord(cx->t[4], s));
    if ((rc = rs.wait(s))) return rc;
    *n_bytes = total;
    *n_rows = n_out;
    st->ms_inflate += elapsed(cx->t[0], cx->t[1]);
    st->ms_kernels += elapsed(cx->t[1], cx->t[2]);
    st->ms_copy += elapsed(cx->t[3], cx->t[4]);
    return CTO_OK;
}

int64_t chunk_budget(int where) {
    if (const char* e = getenv("CTO_CONTAM_CHUNK_BYTES")) { const long long v = atoll(e); if (v > 0) return v; }
    return where ? int64_t(256) << 20 : int64_t(2) << 20;
}

int thread_count(int host_threads) {
    return host_threads > 0 ? std::min(host_threads, 64) : int(std::max(1u, std::min(std::thread::hardware_concurrency(), 16u)));
}

// the contigs a call walks: one, or all in header order
int contigs_of(const char* who, const BamHeader& h, const char* ctg_name, std::vector<int>* tids) {
    for (int t = 0; t < int(h.names.size()); ++t)
        if (!ctg_name || h.names[size_t(t)] == ctg_name) { tids->push_back(t); if (ctg_name) break; }
    CTO_REQUIRE(!ctg_name || !tids->empty(), CTO_EINVAL, "%s: contig %s not in the BAM header", who, ctg_name);
    return CTO_OK;
}

// the windows of one contig as a stack of [a, b) in 16 kb windows, the first on top: a window found too large is halved
std::vector<std::pair<int64_t, int64_t>> window_stack(const std::vector<int64_t>& cuts) {
    std::vector<std::pair<int64_t, int64_t>> todo;
    for (int64_t c = int64_t(cuts.size()) - 1; c-- > 0;) todo.push_back({cuts[size_t(c)], cuts[size_t(c) + 1]});
    return todo;
}

}  // namespace

extern "C" int cto_subsample_keys(const uint8_t* names, const int64_t* off, int64_t n, uint32_t seed, int m, uint32_t* k24, uint8_t* keep) {
    return guarded("cto_subsample_keys", [&]() -> int {
        CTO_REQUIRE(n >= 0 && (n == 0 || (names && off)), CTO_EINVAL, "cto_subsample_keys: null argument");
        CTO_REQUIRE(m >= 0 && m <= 1000, CTO_EINVAL, "cto_subsample_keys: m must be 0 .. 1000 thousandths");
        for (int64_t i = 0; i < n; ++i) {
            CTO_REQUIRE(off[i + 1] >= off[i] && off[i + 1] - off[i] <= 254, CTO_EINVAL, "cto_subsample_keys: a read name has 0 .. 254 bytes");
            const uint32_t k = subsample_key(names + off[i], int(off[i + 1] - off[i]), seed);
            if (k24) k24[i] = k;
            if (keep) keep[i] = subsample_keeps(k, m);
        }
        return CTO_OK;
    });
}

extern "C" int64_t cto_bam_coverage(const char* bam_path, const char* bai_path, const char* ctg_name, int where, int host_threads, void* stream,
                                    cto_cov_row* rows, int64_t cap, cto_contam_stats* stats) {
    int64_t n_rows = 0;
    const int rc = guarded("cto_bam_coverage", [&]() -> int {
        CTO_REQUIRE(bam_path && (rows || cap == 0) && cap >= 0, CTO_EINVAL, "cto_bam_coverage: null argument");
        CTO_REQUIRE(where == 0 || where == 1, CTO_EINVAL, "cto_bam_coverage: where must be 0 (host) or 1 (device)");
        (void)host_threads;                                             // the windows of a contig hand their open spans on: one after the other
        cto_contam_stats st{};
        if (stats) *stats = st;
        BamHeader h;
        std::vector<int> tids;
        int rc;
        if ((rc = contam_read_header("cto_bam_coverage", bam_path, &h)) || (rc = contigs_of("cto_bam_coverage", h, ctg_name, &tids))) return rc;
        CTO_REQUIRE(int64_t(tids.size()) <= cap, CTO_ENOMEM, "cto_bam_coverage: %zu contigs, room for %lld rows", tids.size(), (long long)cap);
        const std::string bai = bai_path ? std::string(bai_path) : std::string(bam_path) + ".bai";
        const char* bams[1] = {bam_path};
        const char* bais[1] = {bai.c_str()};
        ContamCtx* cx = nullptr;
        std::unique_lock<std::mutex> lock;
        hipStream_t s = static_cast<hipStream_t>(stream);
        if (where == 1) {
            cx = &process_wide<ContamCtx>();
            lock = std::unique_lock<std::mutex>(cx->mu);
            for (Event& e : cx->t) if (!e && (rc = e.create())) return rc;
        }
        for (int t : tids) {
            const char* ctg = h.names[size_t(t)].c_str();
            const int64_t L = h.lens[size_t(t)];
            cto_cov_row row{L, 0, t, 0, 0, 0};
            std::vector<int64_t> cuts;
            if ((rc = contam_plan_windows("cto_bam_coverage", bams, bais, 1, ctg, L, chunk_budget(where), &cuts))) return rc;
            auto todo = window_stack(cuts);
            std::vector<int32_t> carry;
            int32_t lo = INT32_MAX, hi = INT32_MIN;
            while (!todo.empty()) {
                const auto [a, b] = todo.back();
                todo.pop_back();
                const int64_t w0 = a * kContamWindow, w1 = b * kContamWindow;
                int64_t bases = 0, counted = 0;
                int32_t mn = 0, mx = 0;
                int outcome = where == 1 ? CHUNK_DONE : CHUNK_NOTHING;
                if (where == 1 && (rc = cov_window_device(cx, bam_path, bai.c_str(), ctg, w0, w1, L, &carry, s, &st, &bases, &mn, &mx, &outcome))) return rc;
                if (outcome == CHUNK_TOO_LARGE) {
                    CTO_REQUIRE(b - a > 1, CTO_EUNSUPPORTED, "cto_bam_coverage: more than 4 GiB of alignment records over one 16 kb window");
                    todo.push_back({a + (b - a) / 2, b});
                    todo.push_back({a, a + (b - a) / 2});
                    continue;
                }
                ++st.n_chunks;
                if (outcome != CHUNK_DONE) {
                    const double t0 = now_ms();
                    if ((rc = cov_window_host(bam_path, bai.c_str(), ctg, w0, w1, L, &carry, &bases, &mn, &mx, &counted))) return rc;
                    if (where == 0) st.ms_inflate += now_ms() - t0;
                    st.n_records += counted;
                    st.fallback_chunks += outcome == CHUNK_DAMAGED;
                }
                row.bases += bases;
                lo = std::min(lo, mn);
                hi = std::max(hi, mx);
            }
            if (lo <= hi) { row.min = lo; row.max = hi; }
            rows[n_rows++] = row;
        }
        if (stats) *stats = st;
        return CTO_OK;
    });
    return rc == CTO_OK ? n_rows : rc;
}

extern "C" int cto_bam_mix(const char* tumor_path, const char* tumor_bai, const char* normal_path, const char* normal_bai, const char* ctg_name,
                           int m_tumor, int m_normal, uint32_t seed, const char* out_path, int where, int host_threads, void* stream,
                           cto_contam_stats* stats) {
    return cto_bam_mix_ex(tumor_path, tumor_bai, normal_path, normal_bai, ctg_name, m_tumor, m_normal, seed, out_path, where, host_threads, stream,
                          stats, 0, nullptr);
}

extern "C" int cto_bam_mix_ex(const char* tumor_path, const char* tumor_bai, const char* normal_path, const char* normal_bai, const char* ctg_name,
                              int m_tumor, int m_normal, uint32_t seed, const char* out_path, int where, int host_threads, void* stream,
                              cto_contam_stats* stats, int deflate, cto_deflate_stats* dstats) {
    return guarded("cto_bam_mix", [&]() -> int {
        CTO_REQUIRE(deflate >= 0 && deflate <= 2, CTO_EINVAL, "cto_bam_mix: deflate must be 0 (zlib), 1 (device coder) or 2 (its host restatement)");
        if (dstats) *dstats = cto_deflate_stats{};
        CTO_REQUIRE(tumor_path && normal_path && out_path, CTO_EINVAL, "cto_bam_mix: null argument");
        CTO_REQUIRE(where == 0 || where == 1, CTO_EINVAL, "cto_bam_mix: where must be 0 (host) or 1 (device)");
        CTO_REQUIRE(m_tumor >= 0 && m_tumor <= 1000 && m_normal >= 0 && m_normal <= 1000, CTO_EINVAL,
                    "cto_bam_mix: the proportions are 0 .. 1000 thousandths");
        cto_contam_stats st{};
        if (stats) *stats = st;
        BamHeader h, hn;
        std::vector<int> tids;
        int rc;
        if ((rc = contam_read_header("cto_bam_mix", tumor_path, &h)) || (rc = contam_read_header("cto_bam_mix", normal_path, &hn))) return rc;
        CTO_REQUIRE(h.names.size() == hn.names.size(), CTO_EINVAL, "cto_bam_mix: the reference lists differ: %zu references in %s, %zu in %s",
                    h.names.size(), tumor_path, hn.names.size(), normal_path);
        for (size_t r = 0; r < h.names.size(); ++r) {
            CTO_REQUIRE(h.names[r] == hn.names[r], CTO_EINVAL, "cto_bam_mix: the reference lists differ: reference %zu is %s in %s and %s in %s", r,
                        h.names[r].c_str(), tumor_path, hn.names[r].c_str(), normal_path);
            CTO_REQUIRE(h.lens[r] == hn.lens[r], CTO_EINVAL, "cto_bam_mix: the reference lists differ: %s has length %lld in %s and %lld in %s",
                        h.names[r].c_str(), (long long)h.lens[r], tumor_path, (long long)hn.lens[r], normal_path);
        }
        if ((rc = contigs_of("cto_bam_mix", h, ctg_name, &tids))) return rc;
        const std::string tbai = tumor_bai ? std::string(tumor_bai) : std::string(tumor_path) + ".bai";
        const std::string nbai = normal_bai ? std::string(normal_bai) : std::string(normal_path) + ".bai";
        const char* bams[2] = {tumor_path, normal_path};
        const char* bais[2] = {tbai.c_str(), nbai.c_str()};
        const int m[2] = {m_tumor, m_normal};
        // the window plan reads both indices: a missing one is reported before the output file is opened
        std::vector<std::vector<int64_t>> plans(tids.size());
        for (size_t k = 0; k < tids.size(); ++k)
            if ((rc = contam_plan_windows("cto_bam_mix", bams, bais, 2, h.names[size_t(tids[k])].c_str(), h.lens[size_t(tids[k])], chunk_budget(where),
                                          &plans[k])))
                return rc;
        ContamCtx* cx = nullptr;
        std::unique_lock<std::mutex> lock;
        hipStream_t s = static_cast<hipStream_t>(stream);
        if (where == 1) {
            cx = &process_wide<ContamCtx>();
            lock = std::unique_lock<std::mutex>(cx->mu);
            for (Event& e : cx->t) if (!e && (rc = e.create())) return rc;
        }
        MixWriter wr;
        if ((rc = wr.open(out_path, h, thread_count(host_threads), deflate, stream))) return rc;
        const bool code_here = where == 1 && deflate == 1;           // the stream never comes down: its blocks do
        std::vector<uint8_t> stream_bytes;
        std::vector<MixRow> rows;
        for (size_t k = 0; k < tids.size(); ++k) {
            const int t = tids[k];
            const char* ctg = h.names[size_t(t)].c_str();
            auto todo = window_stack(plans[k]);
            while (!todo.empty()) {
                const auto [a, b] = todo.back();
                todo.pop_back();
                const int64_t w0 = a * kContamWindow, w1 = b * kContamWindow;
                int outcome = where == 1 ? CHUNK_DONE : CHUNK_NOTHING;
                int64_t n_bytes = 0, n_rows = 0;
                MixCounts counts{};
                CodedDown coded;
                if (where == 1 && (rc = mix_window_device(cx, bams, bais, ctg, w0, w1, m, seed, s, &st, &n_bytes, &n_rows, &counts, &outcome,
                                                          code_here ? &wr.pending : nullptr, code_here ? &coded : nullptr, &wr.dst)))
                    return rc;
                if (outcome == CHUNK_TOO_LARGE) {
                    CTO_REQUIRE(b - a > 1, CTO_EUNSUPPORTED, "cto_bam_mix: more than 4 GiB of alignment records over one 16 kb window");
                    todo.push_back({a + (b - a) / 2, b});
                    todo.push_back({a, a + (b - a) / 2});
                    continue;
                }
                ++st.n_chunks;
                if (outcome == CHUNK_DONE && code_here && n_bytes) {
                    if ((rc = wr.append_coded(t, size_t(n_bytes), cx->h_rows.as<MixRow>(), size_t(n_rows), coded.sizes, size_t(coded.n_blocks), coded.blocks,
                                              cx->h_out.as<uint8_t>(), size_t(coded.n_rest))))
                        return rc;
                } else if (outcome == CHUNK_DONE) {
                    if ((rc = wr.append(t, cx->h_out.as<uint8_t>(), size_t(n_bytes), cx->h_rows.as<MixRow>(), size_t(n_rows)))) return rc;
                } else {
                    const double t0 = now_ms();
                    if ((rc = mix_window_host(bams, bais, ctg, w0, w1, m, seed, &stream_bytes, &rows, &counts))) return rc;
                    if (where == 0) st.ms_inflate += now_ms() - t0;
                    st.fallback_chunks += outcome == CHUNK_DAMAGED;
                    if ((rc = wr.append(t, stream_bytes.data(), stream_bytes.size(), rows.data(), rows.size()))) return rc;
                }
                for (int x = 0; x < 2; ++x) { st.candidates[x] += counts.cand[x]; st.kept[x] += counts.kept[x]; }
                st.n_records += counts.kept[0] + counts.kept[1];
            }
        }
        if ((rc = wr.close(&st.out_bytes, &st.out_blocks))) return rc;
        st.ms_write = wr.ms;
        if (stats) *stats = st;
        if (dstats) *dstats = wr.dst;
        return CTO_OK;
    });
}
