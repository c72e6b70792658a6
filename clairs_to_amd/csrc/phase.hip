// Read phasing and haplotagging from a BAM: heterozygous SNP sites of one contig -> phase and phase set per site, haplotype and phase
// set per read - what `longphase phase` and `longphase haplotag` (or whatshap) do between STEP 3 and STEP 4 of run_clairs_to, in one
// pass over the BAM.  cto_phase_reads is the C entry point; the host path (csrc/bam.cpp on bam_host.h) is the plain definition of the
// rules below and the device path in this file is held equal to it, array for array (tests/test_gpu_phase.py).
//
// PARITY UNPINNED against longphase and whatshap: neither program exists on the build or GPU machines.  The rules are the definition;
// tests/test_phase_reads.py holds them against a naive restatement and against simulated truth.  All arithmetic is integer.
//
// Rules (positions 1-based, sites strictly ascending, one REF and one ALT letter each):
//   a. observations.  A read enters exactly as in cto_af_tallies (csrc/aftally.hip) when it overlaps pos[0] .. pos[n - 1].  At every
//      site inside its reference span an M / = / X base that equals REF (upper-cased) observes allele 0, one that equals ALT allele 1;
//      another letter, N, an IUPAC code, a deletion or a reference skip observes nothing; an insertion behind the base changes
//      nothing.  A read is named by the virtual offset of its record.  The sites are cut into chunks under an inflated-byte budget
//      (CTO_PHASE_CHUNK_BYTES); chunk [a, b) reads the stretch pos[a] - 1 .. pos[b] - 1, so the stretches tile the whole; a read that
//      enters several chunks has its observations merged by its name, and each site belongs to one chunk, so nothing counts twice.
//      Result: reads in file order, each with its (site, allele) pairs in ascending site order.
//   b. linkage.  For every read and every pair of its observations at sites a < b with b - a <= K (in site index):
//      link[a][b - a - 1][allele_a != allele_b] += 1.  int32 n x K x 2; no dependence on the order of the reads.
//   c. phase (host, one sequential pass: phase_sites in csrc/bam.cpp).  Site 0 opens block 0 with phase 0.  Site b sums over the phased
//      sites a in [b - K, b - 1] of the open block same (link[a][..][0] when phase[a] == 0, else [..][1]) and flip (the other);
//      T = same + flip.  T < 2: b opens a new block with phase 0.  Else 4 min(same, flip) > T: b stays unphased, casts no votes later
//      and belongs to no block.  Else phase[b] = flip > same and b joins the open block.  PS = position of the block's first site.
//   d. read assignment.  An observation at a phased site votes for haplotype allele ^ phase in that site's block; the read takes the
//      block where it has the most votes (ties: the lowest block); with h1, h2 its votes there HP = 1 when 10 h1 >= 6 (h1 + h2),
//      HP = 2 when 10 h2 >= 6 (h1 + h2), else untagged (0.6 is longphase's default threshold).  PS is that block's.
//
// Device path.  Per chunk the front end is the allele counter's (csrc/allelecount.hip): cto_bam_chunk_span, cto_bgzf_scan, copy up,
// cto_bgzf_inflate, k_crc32_blocks, k_linearise, k_chain, k_parse_ph, k_entered_*, then
//   k_span      one lane per record: the entered read's sites [lo, hi) by binary search, its virtual offset from the block table
//   k_observe   one wave per entered read, the walk of aftally.hip's k_tally: 64 CIGAR operations at a time, prefix sums give every
//               lane its operation's reference and query offsets, every lane serves the sites inside its own operation.  A read owns
//               hi - lo slots (one byte each, 0xff = nothing): slot order is site order, and no two lanes share a slot - no atomics.
// The slots come down, the host merges the chunks' reads (phase_merge), and the merged CSR goes up once for
//   k_link      one wave per read, lanes over its observations, each pairing its own with the ones up to K sites behind it: integer
//               atomicAdds into link
//   k_assign    one lane per read: one pass over its observations - block numbers ascend with the sites, so a read's votes per block
//               are consecutive runs
// with phase_sites on the host between the two.  A chunk that does not inflate, fails a CRC-32 or has a broken record chain is redone
// by the host path (stats.fallback_chunks).
#include <algorithm>
#include <atomic>
#include <chrono>
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

// parse_record (bam_records.h) with cto_af_tallies' filters: unmapped, excluded flags, MAPQ, orphans
__global__ void k_parse_ph(const uint8_t* __restrict__ lin, const uint32_t* __restrict__ rec_off, int n_rec, int tid, int beg0, int end0,
                           int excl_flags, int min_mq, DevRead* __restrict__ reads, Flags* fl) {
    parse_record<false>(lin, rec_off, n_rec, tid, beg0, end0, [=](int flag, int mapq) {
        return !((flag & excl_flags) || (flag & 4) || mapq < min_mq || ((flag & 1) && !(flag & 2))); }, reads, fl);
}

__global__ void k_entered_marks(const DevRead* __restrict__ reads, int n_rec, const Flags* fl, int* __restrict__ mark) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_rec) mark[i] = reads[i].valid && i < fl->stop_idx;
}
__global__ void k_entered_write(const int* __restrict__ mark, const int* __restrict__ at, int n_rec, int* __restrict__ rid) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_rec && mark[i]) rid[at[i]] = i;
}

__device__ __forceinline__ int first_site_ge(const int32_t* __restrict__ pos0, int a, int b, int p) {        // in [a, b], pos0 ascending
    while (a < b) { const int m = (a + b) >> 1; if (pos0[m] >= p) b = m; else a = m + 1; }
    return a;
}

// what comes down per entered read: its name, where its slots start, its first site (chunk-local) and how many sites it spans
struct ReadOut { unsigned long long voff; long long off; int lo, width; };

__global__ void k_span(const DevRead* __restrict__ reads, const int* __restrict__ mark, const int* __restrict__ at, int n_rec,
                       const int32_t* __restrict__ pos0, int n_sites, const int64_t* __restrict__ lin_off, const cto_bgzf_block* __restrict__ blocks,
                       int n_blocks, int* __restrict__ width, ReadOut* __restrict__ ro) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rec) return;
    if (!mark[i]) { width[i] = 0; return; }
    const DevRead r = reads[i];
    const int lo = first_site_ge(pos0, 0, n_sites, r.pos), hi = first_site_ge(pos0, lo, n_sites, r.end);
    width[i] = hi - lo;
    int a = 0, b = n_blocks;                                      // the last block that starts at or before the record
    while (a < b) { const int m = (a + b) >> 1; if (lin_off[m] <= int64_t(r.off)) a = m + 1; else b = m; }
    const int blk = a - 1;
    ReadOut o;
    o.voff = (static_cast<unsigned long long>(blocks[blk].file_off) << 16) | static_cast<unsigned long long>(int64_t(r.off) - lin_off[blk]);
    o.off = 0;
    o.lo = lo;
    o.width = hi - lo;
    ro[at[i]] = o;
}

__global__ __launch_bounds__(256) void k_observe(const uint8_t* __restrict__ lin, const DevRead* __restrict__ reads, const int* __restrict__ rid,
                                                 const Flags* fl, const int32_t* __restrict__ pos0, const uint8_t* __restrict__ codes,
                                                 const long long* __restrict__ woff, ReadOut* __restrict__ ro, uint8_t* __restrict__ slots) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= fl->n_valid) return;
    const int i = rid[j];
    const DevRead r = reads[i];
    const long long off = woff[i];
    const int lo = ro[j].lo, hi = lo + ro[j].width;
    if (lane == 0) ro[j].off = off;
    if (lo == hi) return;
    const int last = pos0[hi - 1];
    const uint8_t* ops = lin + r.ops_off;
    const uint8_t* seq = lin + r.seq_off;
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
        if (!(cons_ref && cons_q)) continue;                      // D, N: nothing
        for (int a = first_site_ge(pos0, lo, hi, op_ref); a < hi && pos0[a] < op_ref + len; ++a) {
            const int q = op_q + (pos0[a] - op_ref);
            const int code = (seq[q >> 1] >> ((~q & 1) << 2)) & 15;
            if (code != 1 && code != 2 && code != 4 && code != 8) continue;
            if (code == codes[2 * a]) slots[off + (a - lo)] = 0;
            else if (code == codes[2 * a + 1]) slots[off + (a - lo)] = 1;
        }
    }
}

__global__ __launch_bounds__(256) void k_link(const long long* __restrict__ off, const int32_t* __restrict__ obs, long long n_reads, int K,
                                              int* __restrict__ link) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_reads) return;
    const long long b = off[r], e = off[r + 1];
    for (long long i = b + lane; i < e; i += 64) {
        const int oi = obs[i], si = oi >> 1;
        for (long long j = i + 1; j < e; ++j) {
            const int oj = obs[j], d = (oj >> 1) - si;
            if (d > K) break;
            atomicAdd(&link[((long long)si * K + (d - 1)) * 2 + ((oi ^ oj) & 1)], 1);
        }
    }
}

__global__ void k_assign(const long long* __restrict__ off, const int32_t* __restrict__ obs, long long n_reads, const int8_t* __restrict__ phase,
                         const int32_t* __restrict__ block, const int32_t* __restrict__ ps, uint8_t* __restrict__ hp, int32_t* __restrict__ rps) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    int best_h1 = 0, best_h2 = 0, best_ps = 0, h1 = 0, h2 = 0, cur = -1, cur_ps = 0;
    for (long long i = off[r]; i < off[r + 1]; ++i) {
        const int o = obs[i], s = o >> 1, ph = phase[s];
        if (ph < 0) continue;
        if (block[s] != cur) {
            if (h1 + h2 > best_h1 + best_h2) { best_h1 = h1; best_h2 = h2; best_ps = cur_ps; }
            cur = block[s]; cur_ps = ps[s]; h1 = h2 = 0;
        }
        if (((o & 1) ^ ph) == 0) ++h1; else ++h2;
    }
    if (h1 + h2 > best_h1 + best_h2) { best_h1 = h1; best_h2 = h2; best_ps = cur_ps; }
    const int t = best_h1 + best_h2;
    const int h = t > 0 && 10 * best_h1 >= 6 * t ? 1 : (t > 0 && 10 * best_h2 >= 6 * t ? 2 : 0);
    hp[r] = uint8_t(h);
    rps[r] = h ? best_ps : 0;
}

struct PhaseCtx {
    std::mutex mu;                                                  // one device call at a time: the buffers outlive the calls
    InflatedSpan span;
    RecordStream rs;
    DevBuf reads, mark, at, rid, width, woff, ro, slots;            // per chunk
    DevBuf csr, site, link, tag;                                    // over the merged reads
    PinBuf h_ro, h_slots, h_csr, h_site, h_link, h_tag;
    Event t[5], u[6];
};

enum { CHUNK_DONE = 0, CHUNK_DAMAGED = 1, CHUNK_NOTHING = 2, CHUNK_TOO_LARGE = 3 };

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
float elapsed(hipEvent_t a, hipEvent_t b) { float ms = 0.f; (void)hipEventElapsedTime(&ms, a, b); return ms; }

// The observations of the sites [a, b) on the device, into *part.  *outcome as in csrc/aftally.hip.
int observe_chunk_device(PhaseCtx* cx, const char* bam_path, const char* bai_path, const char* ctg_name, const PhaseSites& S, int64_t a, int64_t b,
                         const PhaseParams& pr, hipStream_t s, cto_phase_stats* st, PhaseReads* part, int* outcome) {
    *outcome = CHUNK_DONE;
    part->voff.clear(); part->obs.clear(); part->off.assign(1, 0);
    const int64_t n_sites = b - a;
    const int64_t lo = S.pos[a], hi = b < S.n ? int64_t(S.pos[b]) - 1 : int64_t(S.pos[S.n - 1]);
    int64_t fb = 0, fe = 0;
    int rc = cto_bam_chunk_span(bam_path, bai_path, ctg_name, lo, hi, &fb, &fe);
    if (rc != CTO_OK) return rc;
    if (fe <= fb) { *outcome = CHUNK_NOTHING; return CTO_OK; }
    InflatedSpan& span = cx->span;
    RecordStream& rs = cx->rs;
    if ((rc = span.read(bam_path, fb, size_t(fe - fb), "cto_phase_reads: "))) return rc;
    const int64_t n = span.scan();
    if (n == CTO_EINVAL) { *outcome = CHUNK_DAMAGED; return CTO_OK; }
    if (n < 0) return int(n);
    if (n == 0) { *outcome = CHUNK_NOTHING; return CTO_OK; }
    SpanTables tables;
    tables.lay_out(span.blocks(), n);
    const int64_t len = tables.len;
    if (len >= (int64_t(1) << 32) - 65536 || n >= (int64_t(1) << 30)) { *outcome = CHUNK_TOO_LARGE; return CTO_OK; }
    std::vector<uint64_t> voffs;
    int32_t tid = -1;
    const int64_t n_st = record_starts(bam_path, bai_path, ctg_name, lo, hi, fb, fe, &voffs, &tid);
    if (n_st < 0) return int(n_st);
    tables.map_starts(span.blocks(), n, voffs.data(), n_st);
    if (tables.n_chains == 0) { *outcome = CHUNK_NOTHING; return CTO_OK; }
    const size_t ns = size_t(n_sites);
    std::vector<int32_t> pos0(ns);
    std::vector<uint8_t> codes(2 * ns);
    for (size_t i = 0; i < ns; ++i) {
        pos0[i] = S.pos[a + int64_t(i)] - 1;
        codes[2 * i] = uint8_t(phase_base_code(S.ref[a + int64_t(i)]));
        codes[2 * i + 1] = uint8_t(phase_base_code(S.alt[a + int64_t(i)]));
    }
    // ---- copy up + inflate ----
    CTO_HIP(hipEventRecord(cx->t[0], s));
    if ((rc = span.inflate(s))) return rc;
    CTO_HIP(hipEventRecord(cx->t[1], s));
    // ---- the record stream and its boundaries; the sites ride in its upload block ----
    UploadParts extra;
    extra.add(pos0.data(), pos0.size() * 4);
    extra.add(codes.data(), codes.size());
    if ((rc = rs.begin(s, span.d_out.p, span.blocks(), n, tables, extra))) return rc;
    const Flags* hf = rs.h_flags.as<Flags>();
    Flags* const fl = rs.fl;
    const uint8_t* lin = rs.lin.as<uint8_t>();
    st->n_blocks += n;
    st->inflated_bytes += len;
    if (span.first_bad_status() >= 0) { *outcome = CHUNK_DAMAGED; return CTO_OK; }
    if (hf->bad_crc || hf->bad_chain) { *outcome = CHUNK_DAMAGED; return CTO_OK; }
    const int n_rec = hf->n_rec;
    if (n_rec <= 0) { st->ms_inflate += elapsed(cx->t[0], cx->t[1]); return CTO_OK; }
    if ((rc = cx->reads.ensure(size_t(n_rec) * sizeof(DevRead))) || (rc = cx->mark.ensure(size_t(n_rec) * 4)) ||
        (rc = cx->at.ensure(size_t(n_rec + 1) * 4)) || (rc = cx->rid.ensure(size_t(n_rec) * 4)) || (rc = cx->width.ensure(size_t(n_rec) * 4)) ||
        (rc = cx->woff.ensure(size_t(n_rec + 1) * 8)) || (rc = cx->ro.ensure(size_t(n_rec) * sizeof(ReadOut))))
        return rc;
    const unsigned rgrid = unsigned(cdiv(n_rec, 128));
    if ((rc = rs.offsets(s, n_rec))) return rc;
    hipLaunchKernelGGL(k_parse_ph, dim3(rgrid), dim3(128), 0, s, lin, rs.rec_off.as<uint32_t>(), n_rec, tid, int(lo - 1), int(hi), pr.excl_flags,
                       pr.min_mq, cx->reads.as<DevRead>(), fl);
    hipLaunchKernelGGL(k_entered_marks, dim3(rgrid), dim3(128), 0, s, cx->reads.as<DevRead>(), n_rec, fl, cx->mark.as<int>());
    if ((rc = rs.scan(s, cx->mark.as<int>(), n_rec, cx->at.as<int>(), &fl->n_valid))) return rc;
    hipLaunchKernelGGL(k_entered_write, dim3(rgrid), dim3(128), 0, s, cx->mark.as<int>(), cx->at.as<int>(), n_rec, cx->rid.as<int>());
    CTO_HIP(hipEventRecord(cx->t[2], s));
    hipLaunchKernelGGL(k_span, dim3(rgrid), dim3(128), 0, s, cx->reads.as<DevRead>(), cx->mark.as<int>(), cx->at.as<int>(), n_rec,
                       rs.extra<int32_t>(0), int(n_sites), rs.parts.at<int64_t>(rs.up.p, 1), rs.parts.at<cto_bgzf_block>(rs.up.p, 2), int(n),
                       cx->width.as<int>(), cx->ro.as<ReadOut>());
    if ((rc = rs.scan(s, cx->width.as<int>(), n_rec, cx->woff.as<long long>(), &fl->n_entries))) return rc;
    CTO_HIP(hipGetLastError());
    if ((rc = rs.fetch_flags(s))) return rc;
    if (hf->err_idx < hf->stop_idx) { *outcome = CHUNK_DAMAGED; return CTO_OK; }
    const int n_valid = hf->n_valid;
    const long long n_slots = hf->n_entries;
    if (n_valid > 0) {
        const size_t ro_bytes = size_t(n_valid) * sizeof(ReadOut), slot_bytes = size_t(n_slots) + 1;
        if ((rc = cx->slots.ensure(slot_bytes)) || (rc = cx->h_slots.ensure(slot_bytes)) || (rc = cx->h_ro.ensure(ro_bytes))) return rc;
        CTO_HIP(hipMemsetAsync(cx->slots.p, 0xff, slot_bytes, s));
        hipLaunchKernelGGL(k_observe, dim3(unsigned(cdiv(n_valid, 4))), dim3(256), 0, s, lin, cx->reads.as<DevRead>(), cx->rid.as<int>(), fl,
                           rs.extra<int32_t>(0), rs.extra<uint8_t>(1), cx->woff.as<long long>(), cx->ro.as<ReadOut>(), cx->slots.as<uint8_t>());
        CTO_HIP(hipGetLastError());
        CTO_HIP(hipEventRecord(cx->t[3], s));
        CTO_HIP(hipMemcpyAsync(cx->h_ro.p, cx->ro.p, ro_bytes, hipMemcpyDeviceToHost, s));
        CTO_HIP(hipMemcpyAsync(cx->h_slots.p, cx->slots.p, slot_bytes, hipMemcpyDeviceToHost, s));
        CTO_HIP(hipEventRecord(cx->t[4], s));
        if ((rc = rs.wait(s))) return rc;
        st->ms_count += elapsed(cx->t[2], cx->t[3]);
        st->ms_copy += elapsed(cx->t[3], cx->t[4]);
        const ReadOut* ro = cx->h_ro.as<ReadOut>();
        const uint8_t* sl = cx->h_slots.as<uint8_t>();
        part->voff.reserve(size_t(n_valid));
        for (int j = 0; j < n_valid; ++j) {
            part->voff.push_back(ro[j].voff);
            for (int x = 0; x < ro[j].width; ++x) {
                const uint8_t v = sl[ro[j].off + x];
                if (v != 0xff) part->obs.push_back(int32_t((a + ro[j].lo + x) * 2 + v));
            }
            part->off.push_back(int64_t(part->obs.size()));
        }
    }
    st->n_reads_entered += n_valid;
    st->ms_inflate += elapsed(cx->t[0], cx->t[1]);
    st->ms_records += elapsed(cx->t[1], cx->t[2]);
    return CTO_OK;
}

// link counts, the phase pass and the reads' tags over the merged reads, on the device but for the pass
int link_phase_assign_device(PhaseCtx* cx, const PhaseReads& R, const PhaseSites& S, int K, hipStream_t s, int8_t* phase, int32_t* ps,
                             std::vector<int32_t>* link, uint8_t* hp, int32_t* rps, cto_phase_stats* st) {
    const size_t nr = R.voff.size(), no = R.obs.size(), n = size_t(S.n);
    const size_t off_bytes = (nr + 1) * 8, csr_bytes = off_bytes + (no + 1) * 4, link_bytes = n * size_t(K) * 2 * 4;
    const size_t site_bytes = align16(n) + n * 8, tag_bytes = align16(nr) + nr * 4 + 16;
    int rc;
    if ((rc = cx->csr.ensure(csr_bytes)) || (rc = cx->h_csr.ensure(csr_bytes)) || (rc = cx->link.ensure(link_bytes)) ||
        (rc = cx->h_link.ensure(link_bytes)) || (rc = cx->site.ensure(site_bytes)) || (rc = cx->h_site.ensure(site_bytes)) ||
        (rc = cx->tag.ensure(tag_bytes)) || (rc = cx->h_tag.ensure(tag_bytes)))
        return rc;
    memcpy(cx->h_csr.p, R.off.data(), off_bytes);
    if (no) memcpy(cx->h_csr.as<char>() + off_bytes, R.obs.data(), no * 4);
    const long long* d_off = cx->csr.as<long long>();
    const int32_t* d_obs = reinterpret_cast<const int32_t*>(cx->csr.as<char>() + off_bytes);
    CTO_HIP(hipEventRecord(cx->u[0], s));
    CTO_HIP(hipMemcpyAsync(cx->csr.p, cx->h_csr.p, csr_bytes, hipMemcpyHostToDevice, s));
    CTO_HIP(hipMemsetAsync(cx->link.p, 0, link_bytes, s));
    CTO_HIP(hipEventRecord(cx->u[1], s));
    if (nr) hipLaunchKernelGGL(k_link, dim3(unsigned(cdiv(int64_t(nr), 4))), dim3(256), 0, s, d_off, d_obs, (long long)nr, K, cx->link.as<int>());
    CTO_HIP(hipGetLastError());
    CTO_HIP(hipEventRecord(cx->u[2], s));
    CTO_HIP(hipMemcpyAsync(cx->h_link.p, cx->link.p, link_bytes, hipMemcpyDeviceToHost, s));
    CTO_HIP(hipEventRecord(cx->u[3], s));
    if ((rc = cx->rs.init()) || (rc = cx->rs.wait(s))) return rc;
    link->assign(cx->h_link.as<int32_t>(), cx->h_link.as<int32_t>() + n * size_t(K) * 2);
    std::vector<int32_t> block(n);
    int64_t n_blocks = 0;
    const double p0 = now_ms();
    phase_sites(link->data(), S.pos, S.n, K, phase, ps, block.data(), &n_blocks);
    st->ms_phase += now_ms() - p0;
    st->n_phase_blocks = n_blocks;
    st->ms_count += elapsed(cx->u[1], cx->u[2]);
    st->ms_copy += elapsed(cx->u[0], cx->u[1]) + elapsed(cx->u[2], cx->u[3]);
    if (!nr) return CTO_OK;
    char* hs = cx->h_site.as<char>();
    memcpy(hs, phase, n);
    memcpy(hs + align16(n), block.data(), n * 4);
    memcpy(hs + align16(n) + n * 4, ps, n * 4);
    const char* ds = cx->site.as<char>();
    char* dt = cx->tag.as<char>();
    CTO_HIP(hipEventRecord(cx->u[0], s));
    CTO_HIP(hipMemcpyAsync(cx->site.p, hs, site_bytes, hipMemcpyHostToDevice, s));
    CTO_HIP(hipEventRecord(cx->u[1], s));
    hipLaunchKernelGGL(k_assign, dim3(unsigned(cdiv(int64_t(nr), 256))), dim3(256), 0, s, d_off, d_obs, (long long)nr,
                       reinterpret_cast<const int8_t*>(ds), reinterpret_cast<const int32_t*>(ds + align16(n)),
                       reinterpret_cast<const int32_t*>(ds + align16(n) + n * 4), reinterpret_cast<uint8_t*>(dt),
                       reinterpret_cast<int32_t*>(dt + align16(nr)));
    CTO_HIP(hipGetLastError());
    CTO_HIP(hipEventRecord(cx->u[2], s));
    CTO_HIP(hipMemcpyAsync(cx->h_tag.p, cx->tag.p, align16(nr) + nr * 4, hipMemcpyDeviceToHost, s));
    CTO_HIP(hipEventRecord(cx->u[3], s));
    if ((rc = cx->rs.wait(s))) return rc;
    memcpy(hp, cx->h_tag.p, nr);
    memcpy(rps, cx->h_tag.as<char>() + align16(nr), nr * 4);
    st->ms_count += elapsed(cx->u[1], cx->u[2]);
    st->ms_copy += elapsed(cx->u[0], cx->u[1]) + elapsed(cx->u[2], cx->u[3]);
    return CTO_OK;
}

int64_t chunk_budget(int where) {
    if (const char* e = getenv("CTO_PHASE_CHUNK_BYTES")) { const long long v = atoll(e); if (v > 0) return v; }
    return where ? int64_t(256) << 20 : int64_t(2) << 20;
}

template <class T> T* dup_array(const T* src, size_t n) {
    T* p = static_cast<T*>(malloc(std::max<size_t>(n, 1) * sizeof(T)));
    if (!p) throw std::bad_alloc();
    if (n) memcpy(p, src, n * sizeof(T));
    return p;
}

}  // namespace

extern "C" void cto_phase_result_free(cto_phase_result* r) {
    if (!r) return;
    free(r->voff); free(r->obs_off); free(r->obs); free(r->hp); free(r->ps);
    free(r);
}

extern "C" int cto_phase_reads(const char* bam_path, const char* bai_path, const char* ctg_name, const int32_t* pos, const uint8_t* ref,
                               const uint8_t* alt, int64_t n, int min_mq, int excl_flags, int link_span, int where, int host_threads, void* stream,
                               int8_t* phase, int32_t* ps, int32_t* link_out, cto_phase_result** out, cto_phase_stats* stats) {
    return guarded("cto_phase_reads", [&]() -> int {
        CTO_REQUIRE(bam_path && ctg_name && out && n >= 0 && (n == 0 || (pos && ref && alt && phase && ps)), CTO_EINVAL,
                    "cto_phase_reads: null argument");
        CTO_REQUIRE(where == 0 || where == 1, CTO_EINVAL, "cto_phase_reads: where must be 0 (host) or 1 (device)");
        CTO_REQUIRE(link_span >= 1 && link_span <= CTO_PHASE_MAX_LINK_SPAN, CTO_EINVAL, "cto_phase_reads: link_span must be 1 .. %d",
                    CTO_PHASE_MAX_LINK_SPAN);
        CTO_REQUIRE(n < (int64_t(1) << 30), CTO_EUNSUPPORTED, "cto_phase_reads: more than 2^30 sites");
        *out = nullptr;
        cto_phase_stats st{};
        if (stats) *stats = st;
        PhaseReads R;
        std::vector<uint8_t> hp;
        std::vector<int32_t> rps;
        if (n > 0) {
            CTO_REQUIRE(pos[0] >= 1, CTO_EINVAL, "cto_phase_reads: positions are 1-based");
            for (int64_t i = 1; i < n; ++i) CTO_REQUIRE(pos[i] > pos[i - 1], CTO_EINVAL, "cto_phase_reads: positions must be strictly ascending");
            const PhaseSites S{pos, ref, alt, n};
            const PhaseParams pr{min_mq, excl_flags, link_span};
            const int K = link_span;
            std::vector<int64_t> cuts;
            int rc = allele_plan_chunks(bam_path, bai_path, ctg_name, pos, n, chunk_budget(where), &cuts);
            if (rc != CTO_OK) return rc;
            std::vector<std::pair<int64_t, int64_t>> todo;      // [first, last) site index, a stack: a chunk found too large is halved
            for (int64_t c = int64_t(cuts.size()) - 1; c-- > 0;) todo.push_back({cuts[size_t(c)], cuts[size_t(c) + 1]});
            std::vector<PhaseReads> parts;
            std::vector<int32_t> link;
            if (where == 0) {
                const int64_t n_chunks = int64_t(todo.size());
                std::reverse(todo.begin(), todo.end());
                parts.resize(size_t(n_chunks));
                unsigned nt = host_threads > 0 ? unsigned(host_threads) : std::max(1u, std::min(std::thread::hardware_concurrency(), 32u));
                nt = unsigned(std::max<int64_t>(1, std::min<int64_t>(nt, n_chunks)));
                std::atomic<int64_t> next{0};
                std::vector<int> rcs(nt, CTO_OK);
                std::vector<std::string> errs(nt);
                std::vector<double> ms(nt, 0.0);
                auto work = [&](unsigned t) {
                    for (int64_t c; (c = next.fetch_add(1)) < n_chunks;) {
                        double m = 0;
                        const int r = guarded("cto_phase_reads", [&] {
                            return phase_observe_host_range(bam_path, bai_path, ctg_name, S, todo[size_t(c)].first, todo[size_t(c)].second, pr,
                                                            &parts[size_t(c)], &m);
                        });
                        if (r != CTO_OK) { if (rcs[t] == CTO_OK) { rcs[t] = r; errs[t] = cto_last_error(); } continue; }
                        ms[t] += m;
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
                    st.ms_records += ms[t];
                }
                st.n_chunks = n_chunks;
                for (const PhaseReads& p : parts) st.n_reads_entered += int64_t(p.voff.size());
                phase_merge(parts, &R, &st.n_merged_reads);
                hp.resize(R.voff.size());
                rps.resize(R.voff.size());
                link.resize(size_t(n) * size_t(K) * 2);
                std::vector<int32_t> block(static_cast<size_t>(n));
                const double c0 = now_ms();
                phase_link_host(R, n, K, link.data());
                const double c1 = now_ms();
                phase_sites(link.data(), pos, n, K, phase, ps, block.data(), &st.n_phase_blocks);
                const double c2 = now_ms();
                phase_assign_host(R, phase, block.data(), ps, hp.data(), rps.data());
                st.ms_count += c1 - c0 + now_ms() - c2;
                st.ms_phase += c2 - c1;
            } else {
                PhaseCtx& cx = process_wide<PhaseCtx>();
                std::lock_guard<std::mutex> lock(cx.mu);
                for (Event& e : cx.t) if (!e && (rc = e.create())) return rc;
                for (Event& e : cx.u) if (!e && (rc = e.create())) return rc;
                hipStream_t s = static_cast<hipStream_t>(stream);
                while (!todo.empty()) {
                    const auto [a, b] = todo.back();
                    todo.pop_back();
                    int outcome = CHUNK_DONE;
                    parts.emplace_back();
                    if ((rc = observe_chunk_device(&cx, bam_path, bai_path, ctg_name, S, a, b, pr, s, &st, &parts.back(), &outcome))) return rc;
                    if (outcome == CHUNK_TOO_LARGE) {
                        CTO_REQUIRE(b - a > 1, CTO_EUNSUPPORTED, "cto_phase_reads: more than 4 GiB of alignment records over one site");
                        parts.pop_back();
                        todo.push_back({a + (b - a) / 2, b});
                        todo.push_back({a, a + (b - a) / 2});
                        continue;
                    }
                    ++st.n_chunks;
                    if (outcome != CHUNK_DONE) {
                        if ((rc = phase_observe_host_range(bam_path, bai_path, ctg_name, S, a, b, pr, &parts.back(), nullptr))) return rc;
                        st.n_reads_entered += int64_t(parts.back().voff.size());
                        st.fallback_chunks += outcome == CHUNK_DAMAGED;
                    }
                }
                phase_merge(parts, &R, &st.n_merged_reads);
                hp.resize(R.voff.size());
                rps.resize(R.voff.size());
                if ((rc = link_phase_assign_device(&cx, R, S, K, s, phase, ps, &link, hp.data(), rps.data(), &st))) return rc;
            }
            if (link_out) memcpy(link_out, link.data(), link.size() * sizeof(int32_t));
        }
        cto_phase_result* res = static_cast<cto_phase_result*>(calloc(1, sizeof(cto_phase_result)));
        if (!res) throw std::bad_alloc();
        try {
            res->n_reads = int64_t(R.voff.size());
            res->n_obs = int64_t(R.obs.size());
            res->voff = dup_array<uint64_t>(R.voff.data(), R.voff.size());
            res->obs_off = dup_array<int64_t>(R.off.data(), R.off.size());
            res->obs = dup_array<int32_t>(R.obs.data(), R.obs.size());
            res->hp = dup_array<uint8_t>(hp.data(), hp.size());
            res->ps = dup_array<int32_t>(rps.data(), rps.size());
        } catch (...) {
            cto_phase_result_free(res);
            throw;
        }
        *out = res;
        if (stats) *stats = st;
        return CTO_OK;
    });
}
