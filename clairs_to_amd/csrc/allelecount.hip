// Per-locus A / C / G / T counts from a BAM: what
//   alleleCounter -b BAM -l LOCI -o OUT -m <min_bq> -q <min_mq> -f <req_flags> -F <excl_flags> [--dense-snps]
// (the first command of the reference's Verdict step, src/cna_germline_tagging.py:56-71; a compiled htslib program) counts for the
// loci of one contig.  cto_allele_counts is the C entry point; the host path (csrc/bam.cpp on bam_host.h: allele_counts_host_range) is the plain
// definition of the rules below and the device path in this file is held equal to it, count for count (tests/test_gpu_allele_counter.py).
//
// PARITY UNPINNED against alleleCounter: there is no htslib on the build or GPU machines, so the program cannot be built and run there.
// Three of the rules below are taken from htslib's behaviour as known, not from a run (marked [unpinned]); tools/pin_allelecounter.sh
// compares with the real program wherever one is installed.
//
// Rules (restated from allele_counter/c/src/bam_access.c:113-161, 300-410 and alleleCounter.c:196-300, 312-325, 429-443; positions
// 1-based):
//   * a read overlapping ctg:first_locus-last_locus enters the pile-up unless
//       - MAPQ < min_mq, or (flag & excl_flags) != 0, or (flag & req_flags) != req_flags;
//       - req_flags has bit 2 (proper pair) and the mate-reverse bit equals the reverse bit (the program's F/R orientation check);
//       - flag & 1796 (UNMAP | SECONDARY | QCFAIL | DUP): the mask htslib's pile-up iterator applies of its own, on top of -F, so
//         duplicates and QC failures are dropped even under -F 0 [unpinned];
//       - its CIGAR is empty;
//   * there is no depth cap (the program sets the iterator's limit to 10^9);
//   * at a locus the entered reads whose reference span covers it are visited in file order; for each
//       is_del  the locus falls into a D or an N operation;
//       q       the query index at the locus; inside D / N the query offset at the start of that operation, i.e. the first base behind
//               the deletion [unpinned];
//       c       the 4-bit base code at q, bq the quality byte at q - a missing quality string is 0xff bytes and reads as 255
//               [unpinned] (q == l_seq, a CIGAR that ends in D / N: c = 0, bq = 0);
//       first read of its name that covers the locus: c is remembered for the name, the read counts iff !is_del && bq >= min_bq;
//       later read of that name: counts iff !is_del && bq >= min_bq && c != the c remembered for the FIRST one - whatever the first
//               one's own deletion state or quality was; a third read is still compared with the first;
//       a counting read adds 1 to A, C, G or T for code 1, 2, 4 or 8, nothing for any other code.
// Deviations: records whose CIGAR does not consume exactly l_seq query bases, or no reference base at all, are skipped (htslib
// would pile them up with what its own accessors make of them); CRAM and the 10x mode are not read.
//
// Device path.  The loci are cut into chunks by span (allele_plan_chunks: the linear index gives the compressed bytes under a span;
// one chunk's inflated bytes are to stay within a budget, 256 MiB unless CTO_ALLELE_CHUNK_BYTES says otherwise - a sixteenth of what
// the 32-bit record offsets reach, which is the room the estimate has to be wrong in; compressed input, inflated slots and the
// linear record stream are grow-only buffers of 1/4, 1 and 1 budget).  A locus belongs to one chunk and a chunk loads every read
// that overlaps its span, so nothing crosses chunks and all reads of a name that cover a locus are in its chunk.  Per chunk, on
// the caller's stream:
//   cto_bam_chunk_span, cto_bgzf_scan, copy up, cto_bgzf_inflate (inflated_span.h: shared with the chunk pipeline)
//   k_crc32_blocks, k_linearise, k_chain (bam_records.h's RecordStream: shared with the column pile-up)
//   k_parse_ac      one lane per record: the filters above, CIGAR lengths (CG:B,I too), the span test
//   k_entered_*     entered reads in file order (scan.h)
//   k_name_hash / k_name_insert / k_name_link
//                   64-bit FNV-1a of every entered read's name; every read takes a slot of its own in an open-addressed table in HBM
//                   (linear probing from its hash, half full at most) - an occupant with the same hash met on the way raises `dup`;
//                   then every read walks its cluster for the nearest EARLIER read whose name is the same byte for byte: prev_same.
//                   The link pass returns at once when no entered read is paired and no two hashes are equal (long-read BAMs).
//                   A probe sequence longer than NAME_PROBE_LIMIT (many reads of one name) hands the chunk to the host path.
//   k_count         one wave per entered read: binary search of the chunk's loci for [pos, end), then one pass over the CIGAR, 64
//                   operations at a time (prefix sums give every lane its operation's reference and query offsets), every lane
//                   serving the loci inside its own operation.  With links, the lane follows prev_same back to the earliest linked
//                   read that covers the locus and takes that read's base there by a walk of its CIGAR.  Counts are integer
//                   atomicAdds on counts[locus][base] in HBM: the result does not depend on order.  (Global atomics, not an LDS
//                   histogram per loci tile: work is dealt by read and a locus takes about `depth` adds spread over the whole
//                   kernel.  The choice is NOT MEASURED: it holds if k_count is a small part of a chunk, which only the ms_inflate /
//                   ms_records / ms_count of tools/allele_bench.py on a device can show - DESIGN.md records them once they exist.)
// Counts come down once per chunk.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "bam_records.h"
#include "common.h"
#include "hip_buffers.h"
#include "inflated_span.h"
#include "pack_internal.h"
#include "scan.h"

using namespace cto;

namespace {

struct AcFlags { int dup, crowded; };
// Longest probe sequence the name table walks.  Linear probing in a table at most half full keeps clusters to a few tens of slots
// unless many entered reads share one name (BAMs with stripped names, `*`): they all probe from one home slot, and insert, link and
// the chain walk of k_count would each be quadratic in their number.  Such a chunk raises `crowded` and is counted by the host path
// (a hash map by name); it is not a damaged chunk.
constexpr unsigned NAME_PROBE_LIMIT = 1024;

// parse_record (bam_records.h) with the allele counter's filters; paired_idx = first entered record with flag bit 1
__global__ void k_parse_ac(const uint8_t* __restrict__ lin, const uint32_t* __restrict__ rec_off, int n_rec, int tid, int beg0, int end0,
                           AlleleParams pr, DevRead* __restrict__ reads, Flags* fl) {
    parse_record<false>(lin, rec_off, n_rec, tid, beg0, end0, [=](int flag, int mapq) {
        return !(mapq < pr.min_mq || (flag & pr.excl_flags) || (flag & pr.req_flags) != pr.req_flags ||
                 ((pr.req_flags & 2) && (((flag & 32) != 0) == ((flag & 16) != 0))) || (flag & 1796)); }, reads, fl);
}

// entered = valid and in front of the record that ended the scan; their exclusive scan places them in file order
__global__ void k_entered_marks(const DevRead* __restrict__ reads, int n_rec, const Flags* fl, int* __restrict__ mark) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_rec) mark[i] = reads[i].valid && i < fl->stop_idx;
}
__global__ void k_entered_write(const int* __restrict__ mark, const int* __restrict__ at, int n_rec, int* __restrict__ rid) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_rec && mark[i]) rid[at[i]] = i;
}

__global__ void k_name_hash(const uint8_t* __restrict__ lin, const DevRead* __restrict__ reads, const int* __restrict__ rid, const Flags* fl,
                            unsigned long long* __restrict__ hash) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= fl->n_valid) return;
    const uint8_t* b = lin + reads[rid[j]].off + 4;
    const int l_name = b[8];
    unsigned long long h = 14695981039346656037ull;
    for (int k = 0; k < l_name; ++k) h = (h ^ b[32 + k]) * 1099511628211ull;
    hash[j] = h;
}
// every entered read takes a slot of its own (table = -1 everywhere before); an occupant with the same hash is met by whichever of the
// two came second - it probes from the same home slot
__global__ void k_name_insert(const unsigned long long* __restrict__ hash, const Flags* fl, int* __restrict__ table, unsigned mask, AcFlags* af) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= fl->n_valid) return;
    const unsigned long long h = hash[j];
    unsigned s = unsigned(h) & mask;
    for (unsigned n = 0; n < NAME_PROBE_LIMIT; ++n, s = (s + 1) & mask) {
        const int old = atomicCAS(&table[s], -1, j);
        if (old == -1) return;
        if (hash[old] == h) af->dup = 1;
    }
    af->crowded = 1;
}
__global__ void k_name_link(const uint8_t* __restrict__ lin, const DevRead* __restrict__ reads, const int* __restrict__ rid, const Flags* fl,
                            const unsigned long long* __restrict__ hash, const int* __restrict__ table, unsigned mask, const AcFlags* af,
                            int* __restrict__ prev_same) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= fl->n_valid) return;
    if (af->crowded) return;                                            // the host path takes the chunk
    if (!(fl->paired_idx < fl->stop_idx) && !af->dup) return;          // no links: k_count does not look at prev_same either
    const unsigned long long h = hash[j];
    const uint8_t* mine = lin + reads[rid[j]].off + 4;
    const int l_name = mine[8];
    int best = -1;
    for (unsigned s = unsigned(h) & mask;; s = (s + 1) & mask) {
        const int o = table[s];
        if (o == -1) break;
        if (o >= j || o <= best || hash[o] != h) continue;
        const uint8_t* theirs = lin + reads[rid[o]].off + 4;
        if (theirs[8] != l_name) continue;
        bool same = true;
        for (int k = 0; k < l_name && same; ++k) same = theirs[32 + k] == mine[32 + k];
        if (same) best = o;
    }
    prev_same[j] = best;
}

__device__ __forceinline__ int first_locus_ge(const int32_t* __restrict__ loci, int a, int b, int p) {      // in [a, b], loci 0-based ascending
    while (a < b) { const int m = (a + b) >> 1; if (loci[m] >= p) b = m; else a = m + 1; }
    return a;
}

// base code of read r at 0-based reference position p (inside its span), by the rules above: a serial walk (linked reads are short)
__device__ int code_at(const uint8_t* __restrict__ lin, const DevRead& r, int p) {
    const uint8_t* ops = lin + r.ops_off;
    int rp = r.pos, qp = 0;
    for (int k = 0; k < r.n_ops; ++k) {
        const uint32_t c = ld32(ops + size_t(k) * 4);
        const int opc = int(c & 15), len = int(c >> 4);
        const bool cons_ref = opc == 0 || opc == 2 || opc == 3 || opc == 7 || opc == 8;
        const bool cons_q = opc == 0 || opc == 1 || opc == 4 || opc == 7 || opc == 8;
        if (cons_ref && p < rp + len) {
            const int q = (opc == 2 || opc == 3) ? qp : qp + (p - rp);
            return q < r.l_seq ? (lin[r.seq_off + (q >> 1)] >> ((~q & 1) << 2)) & 15 : 0;
        }
        if (cons_ref) rp += len;
        if (cons_q) qp += len;
    }
    return 0;
}

__global__ __launch_bounds__(256) void k_count(const uint8_t* __restrict__ lin, const DevRead* __restrict__ reads, const int* __restrict__ rid,
                                               const Flags* fl, const AcFlags* af, const int* __restrict__ prev_same,
                                               const int32_t* __restrict__ loci, int n_loci, int min_bq, int* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= fl->n_valid || af->crowded) return;
    const DevRead r = reads[rid[j]];
    const int lo = first_locus_ge(loci, 0, n_loci, r.pos), hi = first_locus_ge(loci, lo, n_loci, r.end);
    if (lo == hi) return;
    const bool links = (fl->paired_idx < fl->stop_idx) || af->dup;
    const int prev = links ? prev_same[j] : -1;
    const int last = loci[hi - 1];
    const uint8_t* ops = lin + r.ops_off;
    const uint8_t* seq = lin + r.seq_off;
    const uint8_t* qual = lin + r.qual_off;
    int ref_carry = r.pos, q_carry = 0;
    for (int k0 = 0; k0 < r.n_ops && ref_carry <= last; k0 += 64) {
        const int k = k0 + lane;
        uint32_t c = 0;
        if (k < r.n_ops) c = ld32(ops + size_t(k) * 4);
        const int opc = int(c & 15), len = int(c >> 4);
        const bool cons_ref = k < r.n_ops && (opc == 0 || opc == 2 || opc == 3 || opc == 7 || opc == 8);
        const bool cons_q = k < r.n_ops && (opc == 0 || opc == 1 || opc == 4 || opc == 7 || opc == 8);
        int rs = cons_ref ? len : 0, qs = cons_q ? len : 0;
        const int rl = rs, ql = qs;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int a = __shfl_up(rs, d), b = __shfl_up(qs, d);
            if (lane >= d) { rs += a; qs += b; }
        }
        const int op_ref = ref_carry + rs - rl, op_q = q_carry + qs - ql;
        ref_carry += __shfl(rs, 63);
        q_carry += __shfl(qs, 63);
        if (!cons_ref) continue;
        const bool is_del = opc == 2 || opc == 3;
        for (int a = first_locus_ge(loci, lo, hi, op_ref); a < hi && loci[a] < op_ref + len; ++a) {
            const int p = loci[a];
            const int q = is_del ? op_q : op_q + (p - op_ref);
            const int code = q < r.l_seq ? (seq[q >> 1] >> ((~q & 1) << 2)) & 15 : 0;
            const int bq = q < r.l_seq ? int(qual[q]) : 0;
            bool counts_here = !is_del && bq >= min_bq;
            if (prev >= 0 && counts_here) {
                int first = -1;                                     // the earliest linked read that covers the locus
                for (int x = prev; x >= 0; x = prev_same[x]) {
                    const DevRead& e = reads[rid[x]];
                    if (e.pos <= p && p < e.end) first = x;
                }
                if (first >= 0 && code_at(lin, reads[rid[first]], p) == code) counts_here = false;
            }
            if (counts_here) {
                const int slot = code == 1 ? 0 : (code == 2 ? 1 : (code == 4 ? 2 : (code == 8 ? 3 : -1)));
                if (slot >= 0) atomicAdd(&counts[size_t(a) * 4 + slot], 1);
            }
        }
    }
}

struct AlleleCtx {
    std::mutex mu;                                                  // one device call at a time: the buffers outlive the calls
    InflatedSpan span;                                              // the chunk's bytes -> inflated blocks (inflated_span.h)
    RecordStream rs;                                                // -> record offsets (bam_records.h); the loci ride in its upload block
    DevBuf reads, mark, at, rid, hash, table, prev, counts, aflags;
    PinBuf h_aflags, h_counts;
    Event t[4];
};

enum { CHUNK_DONE = 0, CHUNK_DAMAGED = 1, CHUNK_NOTHING = 2, CHUNK_TOO_LARGE = 3, CHUNK_CROWDED = 4 };

// One chunk of loci on the device.  *outcome: CHUNK_DONE (counts written), CHUNK_DAMAGED (the input does not hold up: the caller
// redoes the chunk on the host), CHUNK_NOTHING (no whole BGZF block in the span: likewise, but nothing is wrong), CHUNK_TOO_LARGE
// (more inflated bytes than 32-bit offsets reach: the caller halves the chunk), CHUNK_CROWDED (NAME_PROBE_LIMIT: to the host path).
int count_chunk_device(AlleleCtx* cx, const char* bam_path, const char* bai_path, const char* ctg_name, const int32_t* loci, int64_t n_loci,
                       const AlleleParams& pr, hipStream_t s, int32_t* counts, cto_allele_stats* st, int* outcome) {
    *outcome = CHUNK_DONE;
    const int64_t lo = loci[0], hi = loci[n_loci - 1];
    int64_t fb = 0, fe = 0;
    int rc = cto_bam_chunk_span(bam_path, bai_path, ctg_name, lo, hi, &fb, &fe);
    if (rc != CTO_OK) return rc;
    if (fe <= fb) { *outcome = CHUNK_NOTHING; return CTO_OK; }
    InflatedSpan& span = cx->span;
    RecordStream& rs = cx->rs;
    if ((rc = span.read(bam_path, fb, size_t(fe - fb), "cto_allele_counts: "))) return rc;
    const int64_t n = span.scan();
    if (n == CTO_EINVAL) { *outcome = CHUNK_DAMAGED; return CTO_OK; }      // a block header that is none
    if (n < 0) return int(n);
    if (n == 0) { *outcome = CHUNK_NOTHING; return CTO_OK; }
    SpanTables tables;
    tables.lay_out(span.blocks(), n);
    const int64_t len = tables.len;
    if (len >= (int64_t(1) << 32) - 65536 || n >= (int64_t(1) << 30)) { *outcome = CHUNK_TOO_LARGE; return CTO_OK; }
    // record starts the index names inside the span -> offsets into the linear stream
    std::vector<uint64_t> voffs;
    int32_t tid = -1;
    const int64_t n_st = record_starts(bam_path, bai_path, ctg_name, lo, hi, fb, fe, &voffs, &tid);
    if (n_st < 0) return int(n_st);
    tables.map_starts(span.blocks(), n, voffs.data(), n_st);
    if (tables.n_chains == 0) { *outcome = CHUNK_NOTHING; return CTO_OK; }
    std::vector<int32_t> loci0(static_cast<size_t>(n_loci));
    for (int64_t i = 0; i < n_loci; ++i) loci0[size_t(i)] = loci[i] - 1;

    if ((rc = cx->counts.ensure(size_t(n_loci) * 16)) || (rc = cx->h_counts.ensure(size_t(n_loci) * 16)) || (rc = cx->aflags.ensure(sizeof(AcFlags))) ||
        (rc = cx->h_aflags.ensure(sizeof(AcFlags))))
        return rc;
    // ---- copy up + inflate ----
    CTO_HIP(hipEventRecord(cx->t[0], s));
    if ((rc = span.inflate(s))) return rc;
    CTO_HIP(hipEventRecord(cx->t[1], s));
    // ---- the record stream and its boundaries; the loci ride in its upload block ----
    UploadParts extra;
    extra.add(loci0.data(), loci0.size() * 4);
    if ((rc = rs.begin(s, span.d_out.p, span.blocks(), n, tables, extra))) return rc;
    const Flags* hf = rs.h_flags.as<Flags>();
    Flags* const fl = rs.fl;
    const int32_t* d_loci = rs.extra<int32_t>(0);
    const uint8_t* lin = rs.lin.as<uint8_t>();
    st->n_blocks += n;
    st->inflated_bytes += len;
    if (span.first_bad_status() >= 0) { *outcome = CHUNK_DAMAGED; return CTO_OK; }       // the linear stream was built from bytes nobody uses
    if (hf->bad_crc || hf->bad_chain) { *outcome = CHUNK_DAMAGED; return CTO_OK; }
    const int n_rec = hf->n_rec;
    int n_valid = 0;
    CTO_HIP(hipMemsetAsync(cx->counts.p, 0, size_t(n_loci) * 16, s));
    if (n_rec > 0) {
        if ((rc = cx->reads.ensure(size_t(n_rec) * sizeof(DevRead))) || (rc = cx->mark.ensure(size_t(n_rec) * 4)) ||
            (rc = cx->at.ensure(size_t(n_rec + 1) * 4)) || (rc = cx->rid.ensure(size_t(n_rec) * 4)) || (rc = cx->hash.ensure(size_t(n_rec) * 8)) ||
            (rc = cx->prev.ensure(size_t(n_rec) * 4)))
            return rc;
        unsigned tsize = 64;
        while (tsize < 2u * unsigned(n_rec)) tsize <<= 1;
        if ((rc = cx->table.ensure(size_t(tsize) * 4))) return rc;
        const unsigned rgrid = unsigned(cdiv(n_rec, 128));
        if ((rc = rs.offsets(s, n_rec))) return rc;
        hipLaunchKernelGGL(k_parse_ac, dim3(rgrid), dim3(128), 0, s, lin, rs.rec_off.as<uint32_t>(), n_rec, tid, int(lo - 1), int(hi), pr,
                           cx->reads.as<DevRead>(), fl);
        hipLaunchKernelGGL(k_entered_marks, dim3(rgrid), dim3(128), 0, s, cx->reads.as<DevRead>(), n_rec, fl, cx->mark.as<int>());
        if ((rc = rs.scan(s, cx->mark.as<int>(), n_rec, cx->at.as<int>(), &fl->n_valid))) return rc;
        hipLaunchKernelGGL(k_entered_write, dim3(rgrid), dim3(128), 0, s, cx->mark.as<int>(), cx->at.as<int>(), n_rec, cx->rid.as<int>());
        CTO_HIP(hipMemsetAsync(cx->table.p, 0xff, size_t(tsize) * 4, s));
        CTO_HIP(hipMemsetAsync(cx->aflags.p, 0, sizeof(AcFlags), s));
        hipLaunchKernelGGL(k_name_hash, dim3(rgrid), dim3(128), 0, s, lin, cx->reads.as<DevRead>(), cx->rid.as<int>(), fl, cx->hash.as<unsigned long long>());
        hipLaunchKernelGGL(k_name_insert, dim3(rgrid), dim3(128), 0, s, cx->hash.as<unsigned long long>(), fl, cx->table.as<int>(), tsize - 1,
                           cx->aflags.as<AcFlags>());
        hipLaunchKernelGGL(k_name_link, dim3(rgrid), dim3(128), 0, s, lin, cx->reads.as<DevRead>(), cx->rid.as<int>(), fl,
                           cx->hash.as<unsigned long long>(), cx->table.as<int>(), tsize - 1, cx->aflags.as<AcFlags>(), cx->prev.as<int>());
        CTO_HIP(hipEventRecord(cx->t[2], s));
        hipLaunchKernelGGL(k_count, dim3(unsigned(cdiv(n_rec, 4))), dim3(256), 0, s, lin, cx->reads.as<DevRead>(), cx->rid.as<int>(), fl,
                           cx->aflags.as<AcFlags>(), cx->prev.as<int>(), d_loci, int(n_loci), pr.min_bq, cx->counts.as<int>());
        CTO_HIP(hipGetLastError());
        CTO_HIP(hipMemcpyAsync(cx->h_aflags.p, cx->aflags.p, sizeof(AcFlags), hipMemcpyDeviceToHost, s));
    } else {
        CTO_HIP(hipEventRecord(cx->t[2], s));
    }
    CTO_HIP(hipMemcpyAsync(cx->h_counts.p, cx->counts.p, size_t(n_loci) * 16, hipMemcpyDeviceToHost, s));
    if ((rc = rs.copy_flags(s))) return rc;
    CTO_HIP(hipEventRecord(cx->t[3], s));
    if ((rc = rs.wait(s))) return rc;
    if (n_rec > 0) {
        if (hf->err_idx < hf->stop_idx) { *outcome = CHUNK_DAMAGED; return CTO_OK; }
        if (cx->h_aflags.as<AcFlags>()->crowded) { *outcome = CHUNK_CROWDED; return CTO_OK; }
        n_valid = hf->n_valid;
    }
    memcpy(counts, cx->h_counts.p, size_t(n_loci) * 16);
    st->n_reads_entered += n_valid;
    float ms = 0.f;
    CTO_HIP(hipEventElapsedTime(&ms, cx->t[0], cx->t[1])); st->ms_inflate += ms;
    CTO_HIP(hipEventElapsedTime(&ms, cx->t[1], cx->t[2])); st->ms_records += ms;
    CTO_HIP(hipEventElapsedTime(&ms, cx->t[2], cx->t[3])); st->ms_count += ms;
    return CTO_OK;
}

// inflated bytes per chunk: the device path sizes its buffers by it, the host path only needs enough chunks to keep its threads busy
int64_t chunk_budget(int where) {
    if (const char* e = getenv("CTO_ALLELE_CHUNK_BYTES")) { const long long v = atoll(e); if (v > 0) return v; }
    return where ? int64_t(256) << 20 : int64_t(2) << 20;
}

}  // namespace

extern "C" int cto_allele_counts(const char* bam_path, const char* bai_path, const char* ctg_name, const int32_t* loci, int64_t n_loci,
                                 int min_bq, int min_mq, int req_flags, int excl_flags, int where, int host_threads, void* stream,
                                 int32_t* counts, cto_allele_stats* stats) {
    return guarded("cto_allele_counts", [&]() -> int {
        CTO_REQUIRE(bam_path && ctg_name && n_loci >= 0 && (n_loci == 0 || (loci && counts)), CTO_EINVAL, "cto_allele_counts: null argument");
        CTO_REQUIRE(where == 0 || where == 1, CTO_EINVAL, "cto_allele_counts: where must be 0 (host) or 1 (device)");
        cto_allele_stats st{};
        if (stats) *stats = st;
        if (n_loci == 0) return CTO_OK;
        CTO_REQUIRE(loci[0] >= 1, CTO_EINVAL, "cto_allele_counts: loci are 1-based");
        for (int64_t i = 1; i < n_loci; ++i) CTO_REQUIRE(loci[i] > loci[i - 1], CTO_EINVAL, "cto_allele_counts: loci must be strictly ascending");
        const AlleleParams pr{min_bq, min_mq, req_flags, excl_flags};
        std::vector<int64_t> cuts;
        int rc = allele_plan_chunks(bam_path, bai_path, ctg_name, loci, n_loci, chunk_budget(where), &cuts);
        if (rc != CTO_OK) return rc;
        const int64_t n_chunks = int64_t(cuts.size()) - 1;
        if (where == 0) {
            unsigned nt = host_threads > 0 ? unsigned(host_threads) : std::max(1u, std::min(std::thread::hardware_concurrency(), 32u));
            nt = unsigned(std::max<int64_t>(1, std::min<int64_t>(nt, n_chunks)));
            std::atomic<int64_t> next{0};
            std::vector<int> rcs(nt, CTO_OK);
            std::vector<std::string> errs(nt);
            std::vector<cto_allele_stats> sts(nt);
            auto work = [&](unsigned t) {
                for (int64_t c; (c = next.fetch_add(1)) < n_chunks;) {
                    int64_t entered = 0;
                    double ms_r = 0, ms_c = 0;
                    const int r = guarded("cto_allele_counts", [&] {
                        return allele_counts_host_range(bam_path, bai_path, ctg_name, loci + cuts[size_t(c)], cuts[size_t(c) + 1] - cuts[size_t(c)], pr,
                                                        counts + cuts[size_t(c)] * 4, &entered, &ms_r, &ms_c);
                    });
                    if (r != CTO_OK) { if (rcs[t] == CTO_OK) { rcs[t] = r; errs[t] = cto_last_error(); } continue; }
                    sts[t].n_reads_entered += entered;
                    sts[t].ms_records += ms_r;
                    sts[t].ms_count += ms_c;
                }
            };
            if (nt == 1) work(0);
            else {
                std::vector<std::thread> th;
                for (unsigned t = 0; t < nt; ++t) th.emplace_back(work, t);
                for (auto& x : th) x.join();
            }
            for (unsigned t = 0; t < nt; ++t) {
                if (rcs[t] != CTO_OK) { set_error("%s", errs[t].c_str()); return rcs[t]; }
                st.n_reads_entered += sts[t].n_reads_entered;
                st.ms_records += sts[t].ms_records;
                st.ms_count += sts[t].ms_count;
            }
            st.n_chunks = n_chunks;
            if (stats) *stats = st;
            return CTO_OK;
        }
        // ---- device ----
        AlleleCtx& cx = process_wide<AlleleCtx>();
        std::lock_guard<std::mutex> lock(cx.mu);
        for (Event& e : cx.t) if (!e && (rc = e.create())) return rc;
        hipStream_t s = static_cast<hipStream_t>(stream);
        std::vector<std::pair<int64_t, int64_t>> todo;          // [first, last) loci index, a stack: a chunk found too large is halved
        for (int64_t c = n_chunks; c-- > 0;) todo.push_back({cuts[size_t(c)], cuts[size_t(c) + 1]});
        while (!todo.empty()) {
            const auto [a, b] = todo.back();
            todo.pop_back();
            int outcome = CHUNK_DONE;
            if ((rc = count_chunk_device(&cx, bam_path, bai_path, ctg_name, loci + a, b - a, pr, s, counts + a * 4, &st, &outcome))) return rc;
            if (outcome == CHUNK_TOO_LARGE) {
                CTO_REQUIRE(b - a > 1, CTO_EUNSUPPORTED, "cto_allele_counts: more than 4 GiB of alignment records over one locus");
                todo.push_back({a + (b - a) / 2, b});
                todo.push_back({a, a + (b - a) / 2});
                continue;
            }
            ++st.n_chunks;
            if (outcome != CHUNK_DONE) {
                int64_t entered = 0;
                if ((rc = allele_counts_host_range(bam_path, bai_path, ctg_name, loci + a, b - a, pr, counts + a * 4, &entered, nullptr, nullptr))) return rc;
                st.n_reads_entered += entered;
                st.fallback_chunks += outcome == CHUNK_DAMAGED;
            }
        }
        if (stats) *stats = st;
        return CTO_OK;
    });
}
