// Per-variant depth, ALT count and haplotype tallies from a BAM: what the reference's src/cal_af_distribution.py:44-115 reads off one
//   samtools mpileup --min-MQ <min_mq> --min-BQ 0 --excl-flags <excl_flags> [--output-extra HP] BAM -r ctg:pos-pos
// row per truth variant (one samtools process per variant, a character-by-character parse of the row), for all loci of one contig in
// one pass over the BAM.  cto_af_tallies is the C entry point; the host path (csrc/bam.cpp on bam_host.h: af_tallies_host_range) is the
// plain definition of the rules below and the device path in this file is held equal to it, count for count
// (tests/test_gpu_cal_af.py).  The reference's own output is held by tests/golden/cal_af.json.gz (tests/test_cal_af_distribution.py).
//
// PARITY UNPINNED against samtools: there is no htslib on the build or GPU machines, so `samtools mpileup` cannot be run there.  The
// fixture's rows come from a naive Python pile-up (tests/calafutil.py) that states the same rules; every rule below that is taken from
// samtools' behaviour as known, not from a run, is marked [unpinned].  What the reference then does with a row is pinned.
//
// Rules (positions 1-based):
//   * a read enters unless it is unmapped, (flag & excl_flags) != 0, MAPQ < min_mq, it is an orphan (PAIRED without PROPER_PAIR:
//     mpileup without -A), or it has no CIGAR or no SEQ [unpinned] - the acceptance of csrc/bam.cpp:8-33.  Duplicates and QC failures
//     count unless excl_flags names them.  Deviation, as there: records whose CIGAR does not consume exactly l_seq query bases, or no
//     reference base, are skipped.
//   * --min-BQ is 0: every base prints, and mpileup's mate-overlap quality softening changes nothing.  Both mates count [unpinned].
//   * the entered reads whose reference span covers a locus are visited in file order.  Each is a COVER and has one HP value; it gives
//       M / = / X   an ENTRY: the base, upper case, A C G T or N (IUPAC codes and `=` read as N: no reference is given) [unpinned];
//                   the last aligned base of its operation, when the next operation that is not a P is
//                     I   gets the suffix `+` and the inserted bases (upper case; IUPAC codes as they are, `=` as N) [unpinned],
//                     D   gets the suffix `-` and one N per deleted base (no -f: deleted bases print as N);
//                   an insertion that no aligned base of the read precedes (start of read, behind S / N / D) is not reported;
//       D           the entry `*` (`#` on the reverse strand; the reference upper-cases and `*` equals no allele either way);
//       N           no entry (samtools prints `>` / `<`, which the reference's get_base_list skips) - but still an HP value.
//   * depth cap [unpinned]: every locus is its own mpileup run with samtools' default -d 8000; only the first max_depth covers of a
//     locus are looked at, in file order, reference skips included.
//   * depth = number of entries; alt = number of entries equal to the allele (kind / base / del_len / ins bytes of the C call):
//       kind 0  the plain letter `base`, without suffix                 (SNV: ALT)
//       kind 1  `base` + `+` + exactly the given bytes                  (len(REF) == 1 < len(ALT): ALT[0] + '+' + ALT[1:])
//       kind 2  `base` + `-` + del_len x N                              (len(REF) > 1 == len(ALT): REF[0] + '-' + 'N' * (len(REF) - 1))
//       kind 3  nothing                                                 (anything else: the reference compares with ALT itself)
//   * with_hp: zip(base_list, hp_values) pairs entry i with the HP value of cover i - after a reference skip the entries take the HP
//     value of the cover one place ahead of them, and the last covers' values are dropped.  An HP value is the first HP field of an
//     integer type (c C s S i I), printed in decimal; a read without one prints `*` [unpinned]; an HP of another type counts as absent
//     [unpinned].  "1" and "2" select h1 / a1 and h2 / a2; "12" is `in '12'` too and makes the reference raise (IndexError) when an
//     entry is paired with it: CTO_EINVAL with a message; every other value is haplotype 0.  a* counts the paired entries, h* those
//     equal to the allele.  Without with_hp all six stay 0.
//   * a locus no entered read covers gives zeros.
//
// Device path.  Chunks of loci by span under an inflated-byte budget and the front end are the allele counter's (csrc/allelecount.hip;
// the budget is CTO_AF_CHUNK_BYTES here): cto_bam_chunk_span, cto_bgzf_scan, copy up, cto_bgzf_inflate, k_crc32_blocks, k_linearise,
// k_chain, then
//   k_parse_af    one lane per record: mpileup's filter, CIGAR lengths (CG:B,I too), the span test (bam_records.h: parse_record)
//   k_entered_*   entered reads in file order (scan.h)
//   k_hp_class    one lane per entered read: one walk of the auxiliary area, stepping over every field type (B arrays too), to the
//                 first integer HP: 0, 1, 2 or 3 = "raises"
//   k_tally       one wave per entered read: binary search of the chunk's loci for [pos, end), then one pass over the CIGAR, 64
//                 operations at a time (prefix sums give every lane its operation's reference and query offsets), every lane serving
//                 the loci inside its own operation: cover, entry or skip, the comparison with the locus' allele (the letter; the
//                 4-bit packed inserted bases against the ASCII bytes in HBM; the next operation's length), integer atomicAdds into
//                 out[locus][.] and cover[locus].  Without a skip, entry i of a locus is paired with its own read's HP value, so the
//                 result does not depend on order.  (Global atomics as in the allele counter's k_count; measured here: tally and copy down
//                 are 0.08 / 0.11 ms of a 7.7 / 9.0 ms call, tools/cal_af_bench.py)
// What does depend on order is only flagged on the device and recounted on the host, locus by locus (stats.host_loci), never by
// chunk: a covering reference skip under with_hp; a covering HP of 12 (the host decides whether an entry is paired with it);
// cover > max_depth (known once the chunk's covers are down); an insertion allele of more than CTO_AF_MAX_INS = 64 bases - the kernel's
// comparison is a serial loop of one lane, and 64 bases bound it at one pass of a wave; such alleles never reach the kernel.
// A chunk that does not inflate, fails a CRC-32 or has a broken record chain is redone whole by the host (stats.fallback_chunks).
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
#include "hp_class.h"
#include "inflated_span.h"
#include "pack_internal.h"
#include "scan.h"

using namespace cto;

namespace {

// parse_record (bam_records.h) with mpileup's filters: unmapped, excluded flags, MAPQ, orphans
__global__ void k_parse_af(const uint8_t* __restrict__ lin, const uint32_t* __restrict__ rec_off, int n_rec, int tid, int beg0, int end0,
                           int excl_flags, int min_mq, DevRead* __restrict__ reads, Flags* fl) {
    parse_record<false>(lin, rec_off, n_rec, tid, beg0, end0, [=](int flag, int mapq) {
        return !((flag & excl_flags) || (flag & 4) || mapq < min_mq || ((flag & 1) && !(flag & 2))); }, reads, fl);
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

__device__ __forceinline__ int first_locus_ge(const int32_t* __restrict__ loci, int a, int b, int p) {      // in [a, b], loci 0-based ascending
    while (a < b) { const int m = (a + b) >> 1; if (loci[m] >= p) b = m; else a = m + 1; }
    return a;
}

// The chunk's loci on the device: 0-based positions; per locus the deletion length and where its insertion bytes start (n + 1 offsets);
// kind and letter interleaved
struct DevLoci { const int32_t* pos; const int32_t* del_len; const int32_t* ins_off; const uint8_t* kind_base; const char* ins_bytes; int n; };

// tallies: out [n x 8] (depth, alt, h0 h1 h2, a0 a1 a2) | cover [n] | flag [n]
__global__ __launch_bounds__(256) void k_tally(const uint8_t* __restrict__ lin, const DevRead* __restrict__ reads, const int* __restrict__ rid,
                                               const Flags* fl, const uint8_t* __restrict__ hp, DevLoci L, int with_hp, int* __restrict__ out,
                                               int* __restrict__ cover, int* __restrict__ flag) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= fl->n_valid) return;
    const DevRead r = reads[rid[j]];
    const int32_t* __restrict__ loci = L.pos;
    const int lo = first_locus_ge(loci, 0, L.n, r.pos), hi = first_locus_ge(loci, lo, L.n, r.end);
    if (lo == hi) return;
    const int hap = with_hp ? int(hp[j]) : 0;
    const int last = loci[hi - 1];
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
        if (!cons_ref) continue;
        for (int a = first_locus_ge(loci, lo, hi, op_ref); a < hi && loci[a] < op_ref + len; ++a) {
            atomicAdd(&cover[a], 1);
            if (opc == 3) {                                           // N: an HP value without an entry shifts the pairing
                if (with_hp) atomicOr(&flag[a], 1);
                continue;
            }
            if (hap == 3) atomicOr(&flag[a], 1);                      // the host says whether an entry is paired with it
            bool match = false;
            if (opc != 2) {
                const int off = loci[a] - op_ref, q = op_q + off;
                const int code = (seq[q >> 1] >> ((~q & 1) << 2)) & 15;
                const int letter = code == 1 ? 'A' : (code == 2 ? 'C' : (code == 4 ? 'G' : (code == 8 ? 'T' : 'N')));
                int suffix = 0, nlen = 0;
                if (off == len - 1) {                                 // the operation's last base: does an indel follow?
                    int nx = k + 1;
                    uint32_t nc = 0;
                    while (nx < r.n_ops && ((nc = ld32(ops + size_t(nx) * 4)) & 15) == 6) ++nx;     // P
                    if (nx < r.n_ops && ((nc & 15) == 1 || (nc & 15) == 2)) { suffix = int(nc & 15); nlen = int(nc >> 4); }
                }
                const int kind = L.kind_base[2 * a];
                if (int(L.kind_base[2 * a + 1]) == letter) {
                    if (kind == 0) match = suffix == 0;
                    else if (kind == 2) match = suffix == 2 && nlen == L.del_len[a];
                    else if (kind == 1 && suffix == 1 && nlen == L.ins_off[a + 1] - L.ins_off[a]) {
                        const char* want = L.ins_bytes + L.ins_off[a];
                        match = true;
                        for (int x = 0; x < nlen && match; ++x) {
                            const int qq = q + 1 + x;
                            const int ic = (seq[qq >> 1] >> ((~qq & 1) << 2)) & 15;
                            match = "NACMGRSVTWYHKDBN"[ic] == want[x];   // `=` reads as N
                        }
                    }
                }
            }
            int* o = out + size_t(a) * 8;
            atomicAdd(o, 1);
            if (match) atomicAdd(o + 1, 1);
            if (with_hp) {
                const int h = hap == 3 ? 0 : hap;
                atomicAdd(o + 5 + h, 1);
                if (match) atomicAdd(o + 2 + h, 1);
            }
        }
    }
}

struct AfCtx {
    std::mutex mu;                                                  // one device call at a time: the buffers outlive the calls
    InflatedSpan span;                                              // the chunk's bytes -> inflated blocks (inflated_span.h)
    RecordStream rs;                                                // -> record offsets (bam_records.h); the loci ride in its upload block
    DevBuf reads, mark, at, rid, hp, tally;
    PinBuf h_tally;
    Event t[4];
};

enum { CHUNK_DONE = 0, CHUNK_DAMAGED = 1, CHUNK_NOTHING = 2, CHUNK_TOO_LARGE = 3 };

// One chunk of loci [a, b) on the device.  *outcome: CHUNK_DONE (tally = out | cover | flag of the chunk, in cx->h_tally), CHUNK_DAMAGED
// (the input does not hold up: the caller redoes the chunk on the host), CHUNK_NOTHING (no whole BGZF block in the span: likewise, but
// nothing is wrong), CHUNK_TOO_LARGE (more inflated bytes than 32-bit offsets reach: the caller halves the chunk).
int tally_chunk_device(AfCtx* cx, const char* bam_path, const char* bai_path, const char* ctg_name, const AfLoci& L, int64_t a, int64_t b,
                       const AfParams& pr, hipStream_t s, cto_af_stats* st, int* outcome) {
    *outcome = CHUNK_DONE;
    const int64_t n_loci = b - a;
    const int64_t lo = L.pos[a], hi = L.pos[b - 1];
    int64_t fb = 0, fe = 0;
    int rc = cto_bam_chunk_span(bam_path, bai_path, ctg_name, lo, hi, &fb, &fe);
    if (rc != CTO_OK) return rc;
    if (fe <= fb) { *outcome = CHUNK_NOTHING; return CTO_OK; }
    InflatedSpan& span = cx->span;
    RecordStream& rs = cx->rs;
    if ((rc = span.read(bam_path, fb, size_t(fe - fb), "cto_af_tallies: "))) return rc;
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
    // the chunk's loci as the kernel reads them; an insertion allele the kernel does not compare is kind 3 there (the host recounts it)
    const size_t nl = size_t(n_loci);
    std::vector<int32_t> pos0(nl), meta(2 * nl + 1);
    std::vector<uint8_t> kind_base(2 * nl);
    std::string ins;
    for (size_t i = 0; i < nl; ++i) {
        const int64_t g = a + int64_t(i);
        pos0[i] = L.pos[g] - 1;
        int kind = L.kind[g];
        meta[i] = kind == 2 ? L.del_len[g] : 0;
        meta[nl + i] = int32_t(ins.size());
        if (kind == 1) {
            const int64_t il = L.ins_off[g + 1] - L.ins_off[g];
            if (il > CTO_AF_MAX_INS) kind = 3;
            else ins.append(L.ins_bytes + L.ins_off[g], size_t(il));
        }
        kind_base[2 * i] = uint8_t(kind);
        kind_base[2 * i + 1] = L.base[g];
    }
    meta[2 * nl] = int32_t(ins.size());
    const size_t tally_bytes = nl * 10 * sizeof(int32_t);
    if ((rc = cx->tally.ensure(tally_bytes)) || (rc = cx->h_tally.ensure(tally_bytes))) return rc;
    // ---- copy up + inflate ----
    CTO_HIP(hipEventRecord(cx->t[0], s));
    if ((rc = span.inflate(s))) return rc;
    CTO_HIP(hipEventRecord(cx->t[1], s));
    // ---- the record stream and its boundaries; the loci ride in its upload block ----
    UploadParts extra;
    extra.add(pos0.data(), pos0.size() * 4);
    extra.add(meta.data(), meta.size() * 4);
    extra.add(kind_base.data(), kind_base.size());
    extra.add(ins.data(), ins.size());
    if ((rc = rs.begin(s, span.d_out.p, span.blocks(), n, tables, extra))) return rc;
    const Flags* hf = rs.h_flags.as<Flags>();
    Flags* const fl = rs.fl;
    const DevLoci dl{rs.extra<int32_t>(0), rs.extra<int32_t>(1), rs.extra<int32_t>(1) + nl, rs.extra<uint8_t>(2), rs.extra<char>(3), int(n_loci)};
    const uint8_t* lin = rs.lin.as<uint8_t>();
    st->n_blocks += n;
    st->inflated_bytes += len;
    if (span.first_bad_status() >= 0) { *outcome = CHUNK_DAMAGED; return CTO_OK; }       // the linear stream was built from bytes nobody uses
    if (hf->bad_crc || hf->bad_chain) { *outcome = CHUNK_DAMAGED; return CTO_OK; }
    const int n_rec = hf->n_rec;
    int n_valid = 0;
    int* const d_out = cx->tally.as<int>();
    CTO_HIP(hipMemsetAsync(cx->tally.p, 0, tally_bytes, s));
    if (n_rec > 0) {
        if ((rc = cx->reads.ensure(size_t(n_rec) * sizeof(DevRead))) || (rc = cx->mark.ensure(size_t(n_rec) * 4)) ||
            (rc = cx->at.ensure(size_t(n_rec + 1) * 4)) || (rc = cx->rid.ensure(size_t(n_rec) * 4)) || (rc = cx->hp.ensure(size_t(n_rec))))
            return rc;
        const unsigned rgrid = unsigned(cdiv(n_rec, 128));
        if ((rc = rs.offsets(s, n_rec))) return rc;
        hipLaunchKernelGGL(k_parse_af, dim3(rgrid), dim3(128), 0, s, lin, rs.rec_off.as<uint32_t>(), n_rec, tid, int(lo - 1), int(hi), pr.excl_flags,
                           pr.min_mq, cx->reads.as<DevRead>(), fl);
        hipLaunchKernelGGL(k_entered_marks, dim3(rgrid), dim3(128), 0, s, cx->reads.as<DevRead>(), n_rec, fl, cx->mark.as<int>());
        if ((rc = rs.scan(s, cx->mark.as<int>(), n_rec, cx->at.as<int>(), &fl->n_valid))) return rc;
        hipLaunchKernelGGL(k_entered_write, dim3(rgrid), dim3(128), 0, s, cx->mark.as<int>(), cx->at.as<int>(), n_rec, cx->rid.as<int>());
        if (pr.with_hp)
            hipLaunchKernelGGL(k_hp_class, dim3(rgrid), dim3(128), 0, s, lin, cx->reads.as<DevRead>(), cx->rid.as<int>(), fl, cx->hp.as<uint8_t>());
        CTO_HIP(hipEventRecord(cx->t[2], s));
        hipLaunchKernelGGL(k_tally, dim3(unsigned(cdiv(n_rec, 4))), dim3(256), 0, s, lin, cx->reads.as<DevRead>(), cx->rid.as<int>(), fl,
                           cx->hp.as<uint8_t>(), dl, pr.with_hp, d_out, d_out + nl * 8, d_out + nl * 9);
        CTO_HIP(hipGetLastError());
    } else {
        CTO_HIP(hipEventRecord(cx->t[2], s));
    }
    CTO_HIP(hipMemcpyAsync(cx->h_tally.p, cx->tally.p, tally_bytes, hipMemcpyDeviceToHost, s));
    if ((rc = rs.copy_flags(s))) return rc;
    CTO_HIP(hipEventRecord(cx->t[3], s));
    if ((rc = rs.wait(s))) return rc;
    if (n_rec > 0) {
        if (hf->err_idx < hf->stop_idx) { *outcome = CHUNK_DAMAGED; return CTO_OK; }
        n_valid = hf->n_valid;
    }
    st->n_reads_entered += n_valid;
    float ms = 0.f;
    CTO_HIP(hipEventElapsedTime(&ms, cx->t[0], cx->t[1])); st->ms_inflate += ms;
    CTO_HIP(hipEventElapsedTime(&ms, cx->t[1], cx->t[2])); st->ms_records += ms;
    CTO_HIP(hipEventElapsedTime(&ms, cx->t[2], cx->t[3])); st->ms_count += ms;
    return CTO_OK;
}

// inflated bytes per chunk: the device path sizes its buffers by it, the host path only needs enough chunks to keep its threads busy
int64_t chunk_budget(int where) {
    if (const char* e = getenv("CTO_AF_CHUNK_BYTES")) { const long long v = atoll(e); if (v > 0) return v; }
    return where ? int64_t(256) << 20 : int64_t(2) << 20;
}

// the host path over the loci sel[0 .. n), cut where two neighbours lie more than 16 kb (one window of the linear index) apart, so
// that a few scattered loci do not make it read everything between them
int recount_on_host(const char* bam_path, const char* bai_path, const char* ctg_name, const AfLoci& L, const std::vector<int64_t>& sel,
                    const AfParams& pr, int32_t* out) {
    for (size_t i = 0; i < sel.size();) {
        size_t j = i + 1;
        while (j < sel.size() && L.pos[sel[j]] - L.pos[sel[j - 1]] <= 16384) ++j;
        const int rc = af_tallies_host_range(bam_path, bai_path, ctg_name, L, sel.data() + i, int64_t(j - i), pr, out, nullptr, nullptr, nullptr);
        if (rc != CTO_OK) return rc;
        i = j;
    }
    return CTO_OK;
}

}  // namespace

extern "C" int cto_af_tallies(const char* bam_path, const char* bai_path, const char* ctg_name, const int32_t* loci, int64_t n_loci,
                              const uint8_t* kind, const uint8_t* base, const int32_t* del_len, const char* ins_bytes, const int64_t* ins_off,
                              int min_mq, int excl_flags, int max_depth, int with_hp, int where, int host_threads, void* stream, int32_t* out,
                              cto_af_stats* stats) {
    return guarded("cto_af_tallies", [&]() -> int {
        CTO_REQUIRE(bam_path && ctg_name && n_loci >= 0 && (n_loci == 0 || (loci && kind && base && del_len && ins_off && out)), CTO_EINVAL,
                    "cto_af_tallies: null argument");
        CTO_REQUIRE(where == 0 || where == 1, CTO_EINVAL, "cto_af_tallies: where must be 0 (host) or 1 (device)");
        cto_af_stats st{};
        if (stats) *stats = st;
        if (n_loci == 0) return CTO_OK;
        CTO_REQUIRE(loci[0] >= 1, CTO_EINVAL, "cto_af_tallies: loci are 1-based");
        for (int64_t i = 1; i < n_loci; ++i) CTO_REQUIRE(loci[i] > loci[i - 1], CTO_EINVAL, "cto_af_tallies: loci must be strictly ascending");
        CTO_REQUIRE(ins_off[0] >= 0, CTO_EINVAL, "cto_af_tallies: insertion offsets must ascend from 0 or above");
        for (int64_t i = 0; i < n_loci; ++i) {
            CTO_REQUIRE(kind[i] <= 3, CTO_EINVAL, "cto_af_tallies: kind must be 0 .. 3");
            CTO_REQUIRE(ins_off[i + 1] >= ins_off[i] && ins_off[i + 1] - ins_off[i] < (int64_t(1) << 28), CTO_EINVAL,
                        "cto_af_tallies: insertion offsets must ascend");
        }
        CTO_REQUIRE(ins_bytes || ins_off[n_loci] == ins_off[0], CTO_EINVAL, "cto_af_tallies: null argument");
        const AfLoci L{loci, kind, base, del_len, ins_bytes, ins_off};
        const AfParams pr{min_mq, excl_flags, max_depth, with_hp != 0};
        std::vector<int64_t> cuts;
        int rc = allele_plan_chunks(bam_path, bai_path, ctg_name, loci, n_loci, chunk_budget(where), &cuts);
        if (rc != CTO_OK) return rc;
        const int64_t n_chunks = int64_t(cuts.size()) - 1;
        std::vector<int64_t> all(static_cast<size_t>(n_loci));
        for (int64_t i = 0; i < n_loci; ++i) all[size_t(i)] = i;
        if (where == 0) {
            unsigned nt = host_threads > 0 ? unsigned(host_threads) : std::max(1u, std::min(std::thread::hardware_concurrency(), 32u));
            nt = unsigned(std::max<int64_t>(1, std::min<int64_t>(nt, n_chunks)));
            std::atomic<int64_t> next{0};
            std::vector<int> rcs(nt, CTO_OK);
            std::vector<std::string> errs(nt);
            std::vector<cto_af_stats> sts(nt);
            auto work = [&](unsigned t) {
                for (int64_t c; (c = next.fetch_add(1)) < n_chunks;) {
                    int64_t entered = 0;
                    double ms_r = 0, ms_c = 0;
                    const int r = guarded("cto_af_tallies", [&] {
                        return af_tallies_host_range(bam_path, bai_path, ctg_name, L, all.data() + cuts[size_t(c)], cuts[size_t(c) + 1] - cuts[size_t(c)], pr,
                                                     out, &entered, &ms_r, &ms_c);
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
        AfCtx& cx = process_wide<AfCtx>();
        std::lock_guard<std::mutex> lock(cx.mu);
        for (Event& e : cx.t) if (!e && (rc = e.create())) return rc;
        hipStream_t s = static_cast<hipStream_t>(stream);
        std::vector<std::pair<int64_t, int64_t>> todo;          // [first, last) loci index, a stack: a chunk found too large is halved
        for (int64_t c = n_chunks; c-- > 0;) todo.push_back({cuts[size_t(c)], cuts[size_t(c) + 1]});
        std::vector<int64_t> sel;
        while (!todo.empty()) {
            const auto [a, b] = todo.back();
            todo.pop_back();
            int outcome = CHUNK_DONE;
            if ((rc = tally_chunk_device(&cx, bam_path, bai_path, ctg_name, L, a, b, pr, s, &st, &outcome))) return rc;
            if (outcome == CHUNK_TOO_LARGE) {
                CTO_REQUIRE(b - a > 1, CTO_EUNSUPPORTED, "cto_af_tallies: more than 4 GiB of alignment records over one locus");
                todo.push_back({a + (b - a) / 2, b});
                todo.push_back({a, a + (b - a) / 2});
                continue;
            }
            ++st.n_chunks;
            if (outcome != CHUNK_DONE) {
                int64_t entered = 0;
                if ((rc = af_tallies_host_range(bam_path, bai_path, ctg_name, L, all.data() + a, b - a, pr, out, &entered, nullptr, nullptr))) return rc;
                st.n_reads_entered += entered;
                st.fallback_chunks += outcome == CHUNK_DAMAGED;
                continue;
            }
            // the order-free loci are done; the others go to the host path, locus by locus
            const size_t nl = size_t(b - a);
            const int32_t* h = cx.h_tally.as<int32_t>();
            const int32_t *h_cover = h + nl * 8, *h_flag = h + nl * 9;
            sel.clear();
            for (size_t i = 0; i < nl; ++i) {
                const int64_t g = a + int64_t(i);
                const bool long_ins = kind[g] == 1 && ins_off[g + 1] - ins_off[g] > CTO_AF_MAX_INS;
                if (h_flag[i] || long_ins || (max_depth > 0 && h_cover[i] > max_depth)) sel.push_back(g);
                else memcpy(out + g * 8, h + i * 8, 8 * sizeof(int32_t));
            }
            if (!sel.empty() && (rc = recount_on_host(bam_path, bai_path, ctg_name, L, sel, pr, out))) return rc;
            st.host_loci += int64_t(sel.size());
        }
        if (stats) *stats = st;
        return CTO_OK;
    });
}
