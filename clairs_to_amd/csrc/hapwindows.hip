// Haplotype windows from the BAM: the job that csrc/hapfilter.cpp evaluates (cto_hap_evaluate), built from the alignment records
// themselves instead of from the nine-column text of
//   samtools mpileup --min-MQ q --min-BQ q --excl-flags F [-l bed] -r ctg:lo-hi --output-MQ --output-QNAME --output-extra HP
// cto_hap_windows is the C entry point.  The host path (csrc/bam.cpp on bam_host.h: hap_windows_host) is the plain definition of the
// rules below; the device path in this file is held equal to it, record by record (tests/test_gpu_hap_windows.py).  What the
// reference then does with a job is pinned by its own output (tests/golden/hapfilter*.json.gz, reached from a BAM in
// tests/test_hap_windows.py).
//
// PARITY UNPINNED against samtools: there is no htslib on the build or GPU machines.  The fixtures' rows come from
// tests/golden/hapsim.py, which states the same rules; every rule below that rests on samtools' behaviour as known, not on a run,
// is marked [unpinned].
//
// Rules (positions 1-based; a COVER is an entered read over a position, an ENTRY a cover that prints a base):
//   * a read enters unless it is unmapped, (flag & excl_flags) != 0, MAPQ < min_mq, it is an orphan (PAIRED without PROPER_PAIR:
//     mpileup without -A), or it has no CIGAR or no SEQ [unpinned] - the acceptance of csrc/bam.cpp:8-33.  Deviation, as there: records
//     whose CIGAR does not consume exactly l_seq query bases, or no reference base, are skipped.  A CIGAR of more than 65535
//     operations is read from its CG:B,I tag, as htslib does when it reads the record (bam_host.h: lay_out; bam_records.h: record_cigar).
//   * reads are visited in file order.  Depth cap [unpinned]: a read is dropped when max_depth entered reads are still open at its
//     start (htslib's per-file maxcnt, csrc/bam.cpp:23); with a cap the pass therefore starts at the region's start.
//   * M / = / X   an entry: A C G T or N (IUPAC codes and `=` read as N: no reference is given) [unpinned], lower case on the reverse
//                 strand; the last aligned base of its operation, when the next operation that is not a P is
//                   I   carries `+` and the inserted bases in the strand's case (IUPAC codes as they are, `=` as N) [unpinned],
//                   D   carries `-` and one N / n per deleted base (no -f);
//                 an insertion or deletion that no aligned base of the read precedes is not reported (csrc/bam.cpp:17-19);
//     D           the entry `*`; `#` on the reverse strand only with reverse_del (the command line above has no --reverse-del);
//     N           a cover without an entry (samtools prints `>` / `<`, which parse_row skips).
//   * BQ is the quality of the entry's base, of the query base that FOLLOWS a deletion or skip (0 past the read's end), 0 when the
//     record has no qualities (csrc/bam.cpp:15-16, Read::bq) [unpinned]; BQ and MQ are capped at 93.  A cover below min_bq prints
//     nothing: base, `^` / `$`, quality, name and HP go together.
//   * the key of a record is "<qname>_<0|1>", 1 iff its character printed in lower case or as `#` - so a `*` without reverse_del is
//     _0 on a reverse read too, as in the reference, whose quirk it is.
//   * HP: the first HP field of an integer type (k_hp_class): 1 and 2 are the haplotypes; 12 prints two characters and every other
//     value, another type or no field is untagged.  (The view shows '1' / '2' / '*', and '1' with hp_single = 0 for 12, as the text
//     would parse; other untagged values show as '*': no rule reads more of them.)
//   * start / end markers: `^` stands in front of the first position a read covers, `$` behind the last; parse_row's indices - a
//     head cover gives (number of entries before it) - 1 to the start set (-1: "the last record", as the Python did), a tail cover the
//     index of the last entry so far to the end set; the larger set wins, the end set on a tie.
//   * reference skips: names, HP, BQ and MQ are listed per cover, bases per entry, and parse_row pairs them by index - behind a skip the
//     entries take the values of the cover one place ahead.  The host path implements exactly that.
//   * a column with covers but no entry (skips only) is LEFT OUT.  In cto_hap_evaluate no rule tells it from an absent column: every
//     rule loops over the column's records, or over record indices of its start / end list that an empty column cannot satisfy, and
//     the counts it forms are all zero either way.
//
// Device path.  The wanted intervals are cut into pieces of at most 4 kb and the pieces into chunks by span under an inflated-byte
// budget (CTO_HAP_CHUNK_BYTES, 256 MiB); per chunk the front end is the allele counter's (csrc/allelecount.hip): cto_bam_chunk_span,
// cto_bgzf_scan, copy up, cto_bgzf_inflate, k_crc32_blocks, k_linearise, k_chain, then
//   k_parse_hw    one lane per record: mpileup's filter, CIGAR lengths, the span test (bam_records.h: parse_record)
//   k_entered_*   entered reads in file order (scan.h); k_hp_class (hp_class.h); k_name_*: their names, packed
//   k_live        with a cap: one wave per entered read counts the earlier entered reads still open at its start
//   k_walk<0>     count pass, one wave per entered read: the CIGAR 64 operations at a time through prefix sums; every lane looks up
//                 whether its operation meets a wanted interval (binary search); the operations that do are then taken in turn with
//                 the LANES DEALT OVER THE WANTED POSITIONS inside them (a long read has few operations and long M runs).  Integer
//                 atomicAdds count records and indel bytes per column; a printing skip marks its column.
//   scans         records and indel bytes per column -> offsets (scan.h); the totals size the buffers (one trip to the host)
//   k_walk<1>     fill pass: the same walk; a record claims the next slot of its column
//   k_order       one wave per column: the claimed slots ordered by entered-read index (rank by counting: a read has at most one
//                 record in a column), then a prefix sum over the ordered records' indel lengths places their bytes.  Nothing that
//                 comes down depends on the order the claims landed in.
// The record array - already in hap_internal.h's HapRawRec layout - the indel bytes, per-column counts and marks, names and HP classes
// come down once per chunk; the host turns entered index into interned id while it builds the job.
// Counted, never silent (cto_hap_stats): a chunk that does not inflate, fails a CRC-32 or has a broken record chain is redone whole by
// the host (fallback_chunks); so is a chunk in which the depth cap comes into play, and every chunk behind the first under a cap -
// the cap looks at all reads from the region's start (cap_chunks); a column a printing skip covers is rebuilt by the host rule, column
// by column (host_columns); a chunk past 32-bit offsets or 2^30 records is halved.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>
#include "bam_records.h"
#include "common.h"
#include "hap_internal.h"
#include "hip_buffers.h"
#include "hp_class.h"
#include "inflated_span.h"
#include "pack_internal.h"
#include "scan.h"

using namespace cto;

namespace {

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// While a column is filled: a = indel length << 2 | kind (1 ins, 2 del; 0 none), b = query index of the inserted bases.  As k_order
// leaves it: a = indel_off, b = indel_len - HapRawRec.
struct DRec { int32_t read; uint8_t base, bq, mq, mark; int32_t a, b; };
static_assert(sizeof(DRec) == 16 && sizeof(HapRawRec) == 16, "the device record is the raw record");

struct DevIv { const int32_t* lo; const int32_t* hi; const int32_t* base; int n; };      // 0-based [lo, hi); base: columns in front

__global__ void k_parse_hw(const uint8_t* __restrict__ lin, const uint32_t* __restrict__ rec_off, int n_rec, int tid, int beg0, int end0,
                           int excl_flags, int min_mq, DevRead* __restrict__ reads, Flags* fl) {
    parse_record<true>(lin, rec_off, n_rec, tid, beg0, end0, [=](int flag, int mapq) {
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

// name lengths (without the NUL) of the entered reads, and their bytes at the scanned offsets
__global__ void k_name_len(const uint8_t* __restrict__ lin, const DevRead* __restrict__ reads, const int* __restrict__ rid, const Flags* fl,
                           int n_rec, int* __restrict__ nlen) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_rec) return;
    nlen[j] = j < fl->n_valid ? max(0, int(lin[reads[rid[j]].off + 12]) - 1) : 0;
}
__global__ void k_name_copy(const uint8_t* __restrict__ lin, const DevRead* __restrict__ reads, const int* __restrict__ rid, const Flags* fl,
                            const int* __restrict__ noff, char* __restrict__ names) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= fl->n_valid) return;
    const uint8_t* src = lin + reads[rid[j]].off + 36;
    const int n = noff[j + 1] - noff[j];
    for (int i = 0; i < n; ++i) names[noff[j] + i] = char(src[i]);
}

// the depth cap comes into play when max_depth earlier entered reads are still open at some entered read's start
__global__ __launch_bounds__(256) void k_live(const DevRead* __restrict__ reads, const int* __restrict__ rid, Flags* fl, int max_depth) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= fl->n_valid) return;
    const int pos = reads[rid[j]].pos;
    int n = 0;
    for (int i = lane; i < j; i += 64) n += reads[rid[i]].end > pos;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) n += __shfl_xor(n, d);
    if (lane == 0 && n >= max_depth) atomicExch(&fl->deep_col, 1);
}

__device__ __forceinline__ int first_iv(const DevIv& iv, int p) {      // the first interval that ends behind p
    int a = 0, b = iv.n;
    while (a < b) { const int m = (a + b) >> 1; if (iv.hi[m] > p) b = m; else a = m + 1; }
    return a;
}

// One wave per entered read.  FILL = false counts (cnt, ibytes, flag), FILL = true places the records (col_off, cursor, tmp).
template <bool FILL>
__global__ __launch_bounds__(256) void k_walk(const uint8_t* __restrict__ lin, const DevRead* __restrict__ reads, const int* __restrict__ rid,
                                              const Flags* fl, DevIv iv, int min_bq, int reverse_del, int* __restrict__ cnt,
                                              int* __restrict__ ibytes, uint8_t* __restrict__ flag, const long long* __restrict__ col_off,
                                              int* __restrict__ cursor, DRec* __restrict__ tmp) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= fl->n_valid) return;
    const DevRead r = reads[rid[j]];
    const int k_first = first_iv(iv, r.pos);
    if (k_first >= iv.n || iv.lo[k_first] >= r.end) return;
    const int last_want = iv.hi[iv.n - 1];
    const uint8_t* ops = lin + r.ops_off;
    const uint8_t* seq = lin + r.seq_off;
    const uint8_t* qual = lin + r.qual_off;
    const int mq = min(int(r.mapq), 93);
    int ref_carry = r.pos, q_carry = 0;
    for (int k0 = 0; k0 < r.n_ops && ref_carry < last_want; k0 += 64) {
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
        // does this lane's operation meet a wanted interval, and which indel follows it
        int kiv = iv.n;
        bool wants = false;
        if (cons_ref && len > 0) {
            kiv = first_iv(iv, op_ref);
            wants = kiv < iv.n && iv.lo[kiv] < op_ref + len;
        }
        int ind = 0;
        if (wants && opc != 2 && opc != 3) {
            int nx = k + 1;
            uint32_t nc = 0;
            while (nx < r.n_ops && ((nc = ld32(ops + size_t(nx) * 4)) & 15) == 6) ++nx;      // P
            if (nx < r.n_ops && ((nc & 15) == 1 || (nc & 15) == 2)) ind = int(((nc >> 4) << 2) | (nc & 15));
        }
        // the operations that matter in turn, the lanes dealt over the wanted positions inside each
        unsigned long long todo = __ballot(wants);
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int o_ref = __shfl(op_ref, src), o_q = __shfl(op_q, src), o_len = __shfl(len, src), o_opc = __shfl(opc, src);
            const int o_ind = __shfl(ind, src), o_kiv = __shfl(kiv, src);
            const int pend = o_ref + o_len;
            const bool placeholder = o_opc == 2 || o_opc == 3;
            for (int kk = o_kiv; kk < iv.n && iv.lo[kk] < pend; ++kk) {
                const int lo = max(o_ref, iv.lo[kk]), hi = min(pend, iv.hi[kk]);
                for (int p = lo + lane; p < hi; p += 64) {
                    const int q = placeholder ? o_q : o_q + (p - o_ref);
                    const int bq = (r.no_qual || q >= r.l_seq) ? 0 : min(int(qual[q]), 93);
                    if (bq < min_bq) continue;
                    const int col = iv.base[kk] + (p - iv.lo[kk]);
                    if (o_opc == 3) {                     // a printing skip: the host rebuilds the column
                        if (!FILL) flag[col] = 1;
                        continue;
                    }
                    DRec e;
                    e.read = j;
                    e.bq = uint8_t(bq);
                    e.mq = uint8_t(mq);
                    e.mark = uint8_t((p == r.pos ? 1 : 0) | (p == r.end - 1 ? 2 : 0));
                    e.a = 0;
                    e.b = 0;
                    if (o_opc == 2) e.base = uint8_t(r.rev && reverse_del ? '#' : '*');
                    else {
                        const int code = (seq[q >> 1] >> ((~q & 1) << 2)) & 15;
                        const int letter = code == 1 ? 'A' : (code == 2 ? 'C' : (code == 4 ? 'G' : (code == 8 ? 'T' : 'N')));
                        e.base = uint8_t(r.rev ? letter + 32 : letter);
                        if (p == pend - 1 && o_ind) { e.a = o_ind; e.b = q + 1; }
                    }
                    if (!FILL) {
                        atomicAdd(&cnt[col], 1);
                        if (e.a) atomicAdd(&ibytes[col], int(uint32_t(e.a) >> 2) + 1);
                    } else {
                        tmp[col_off[col] + atomicAdd(&cursor[col], 1)] = e;
                    }
                }
            }
        }
    }
}

// One wave per column: file order, then the indel bytes.
__global__ __launch_bounds__(64) void k_order(const uint8_t* __restrict__ lin, const DevRead* __restrict__ reads, const int* __restrict__ rid,
                                              const int* __restrict__ cnt, const long long* __restrict__ col_off,
                                              const long long* __restrict__ ind_off, int n_col, const DRec* __restrict__ tmp,
                                              DRec* __restrict__ out, char* __restrict__ blob) {
    const int lane = threadIdx.x;
    for (int c = blockIdx.x; c < n_col; c += gridDim.x) {
        const int n = cnt[c];
        if (n == 0) continue;
        const long long base = col_off[c];
        for (int i = lane; i < n; i += 64) {
            const DRec e = tmp[base + i];
            int rank = 0;
            for (int m = 0; m < n; ++m) rank += tmp[base + m].read < e.read;
            out[base + rank] = e;
        }
        __syncthreads();
        long long carry = ind_off[c];
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + lane;
            DRec e{};
            int len = 0;
            if (i < n) {
                e = out[base + i];
                if (e.a) len = int(uint32_t(e.a) >> 2) + 1;
            }
            int inc = len;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int u = __shfl_up(inc, d);
                if (lane >= d) inc += u;
            }
            const long long off = carry + inc - len;
            carry += __shfl(inc, 63);
            if (i < n) {
                if (len) {
                    const int kind = e.a & 3, nlen = len - 1;
                    const bool rev = e.base >= 'a' && e.base <= 'z';
                    const uint8_t* seq = lin + reads[rid[e.read]].seq_off;
                    blob[off] = kind == 1 ? '+' : '-';
                    for (int x = 0; x < nlen; ++x) {
                        char ch = 'N';
                        if (kind == 1) {
                            const int qq = e.b + x;
                            ch = "NACMGRSVTWYHKDBN"[(seq[qq >> 1] >> ((~qq & 1) << 2)) & 15];      // `=` prints as N
                        }
                        blob[off + 1 + x] = rev ? char(ch + 32) : ch;
                    }
                }
                e.a = len ? int(off) : 0;
                e.b = len;
                out[base + i] = e;
            }
        }
        __syncthreads();
    }
}

struct HwCtx {
    std::mutex mu;                                                  // one device call at a time: the buffers outlive the calls
    InflatedSpan span;
    RecordStream rs;
    DevBuf reads, mark, at, rid, hp, nlen, noff, names, cnt, ibytes, flag, col_off, ind_off, cursor, tmp, out, blob, totals;
    PinBuf h_tot, h_down;
    Event t[6];
};

struct Piece { int64_t s, e; };      // 0-based [s, e)

enum { CHUNK_DONE = 0, CHUNK_DAMAGED = 1, CHUNK_NOTHING = 2, CHUNK_TOO_LARGE = 3, CHUNK_CAP = 4 };

// One chunk of pieces [a, b) on the device -> *raw (the columns no printing skip covers) and `skipped` (the 0-based positions one
// does).  *outcome as in csrc/aftally.hip, and CHUNK_CAP: the depth cap comes into play, the host redoes the chunk.
int windows_chunk_device(HwCtx* cx, const char* bam_path, const char* bai_path, const char* ctg_name, const std::vector<Piece>& pc, size_t a,
                         size_t b, int64_t lo, const HapWinParams& pr, hipStream_t s, cto_hap_stats* st, HapRaw* raw,
                         std::vector<int64_t>* skipped, int* outcome) {
    *outcome = CHUNK_DONE;
    const int64_t hi = pc[b - 1].e;                                 // lo, hi: 1-based, inclusive
    int64_t fb = 0, fe = 0;
    int rc = cto_bam_chunk_span(bam_path, bai_path, ctg_name, lo, hi, &fb, &fe);
    if (rc != CTO_OK) return rc;
    if (fe <= fb) { *outcome = CHUNK_NOTHING; return CTO_OK; }
    InflatedSpan& span = cx->span;
    RecordStream& rs = cx->rs;
    const double tr0 = now_ms();
    if ((rc = span.read(bam_path, fb, size_t(fe - fb), "cto_hap_windows: "))) return rc;
    st->ms_read += now_ms() - tr0;
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
    // the chunk's pieces as the kernels read them
    const size_t np = b - a;
    std::vector<int32_t> iv_lo(np), iv_hi(np), iv_base(np + 1);
    int64_t n_col64 = 0;
    for (size_t i = 0; i < np; ++i) {
        iv_lo[i] = int32_t(pc[a + i].s);
        iv_hi[i] = int32_t(pc[a + i].e);
        iv_base[i] = int32_t(n_col64);
        n_col64 += pc[a + i].e - pc[a + i].s;
    }
    if (n_col64 >= (int64_t(1) << 30)) { *outcome = CHUNK_TOO_LARGE; return CTO_OK; }
    iv_base[np] = int32_t(n_col64);
    const int n_col = int(n_col64);
    CTO_HIP(hipEventRecord(cx->t[0], s));
    if ((rc = span.inflate(s))) return rc;
    CTO_HIP(hipEventRecord(cx->t[1], s));
    UploadParts extra;
    extra.add(iv_lo.data(), np * 4);
    extra.add(iv_hi.data(), np * 4);
    extra.add(iv_base.data(), (np + 1) * 4);
    if ((rc = rs.begin(s, span.d_out.p, span.blocks(), n, tables, extra))) return rc;
    const Flags* hf = rs.h_flags.as<Flags>();
    Flags* const fl = rs.fl;
    const DevIv iv{rs.extra<int32_t>(0), rs.extra<int32_t>(1), rs.extra<int32_t>(2), int(np)};
    const uint8_t* lin = rs.lin.as<uint8_t>();
    st->n_blocks += n;
    st->inflated_bytes += len;
    if (span.first_bad_status() >= 0) { *outcome = CHUNK_DAMAGED; return CTO_OK; }
    if (hf->bad_crc || hf->bad_chain) { *outcome = CHUNK_DAMAGED; return CTO_OK; }
    const int n_rec = hf->n_rec;
    if (n_rec == 0) { *outcome = CHUNK_NOTHING; return CTO_OK; }
    if ((rc = cx->reads.ensure(size_t(n_rec) * sizeof(DevRead))) || (rc = cx->mark.ensure(size_t(n_rec) * 4)) ||
        (rc = cx->at.ensure(size_t(n_rec + 1) * 4)) || (rc = cx->rid.ensure(size_t(n_rec) * 4)) || (rc = cx->hp.ensure(size_t(n_rec))) ||
        (rc = cx->nlen.ensure(size_t(n_rec) * 4)) || (rc = cx->noff.ensure(size_t(n_rec + 1) * 4)) || (rc = cx->cnt.ensure(size_t(n_col) * 4)) ||
        (rc = cx->ibytes.ensure(size_t(n_col) * 4)) || (rc = cx->cursor.ensure(size_t(n_col) * 4)) || (rc = cx->flag.ensure(size_t(n_col))) ||
        (rc = cx->col_off.ensure(size_t(n_col + 1) * 8)) || (rc = cx->ind_off.ensure(size_t(n_col + 1) * 8)) || (rc = cx->totals.ensure(64)) ||
        (rc = cx->h_tot.ensure(64)))
        return rc;
    DevRead* const d_reads = cx->reads.as<DevRead>();
    int* const d_rid = cx->rid.as<int>();
    long long* const d_tot = cx->totals.as<long long>();     // records, indel bytes, name bytes (as int at [2])
    const unsigned rgrid = unsigned(cdiv(n_rec, 128)), wgrid = unsigned(cdiv(n_rec, 4));
    if ((rc = rs.offsets(s, n_rec))) return rc;
    hipLaunchKernelGGL(k_parse_hw, dim3(rgrid), dim3(128), 0, s, lin, rs.rec_off.as<uint32_t>(), n_rec, tid, int(lo - 1), int(hi), pr.excl_flags,
                       pr.min_mq, d_reads, fl);
    hipLaunchKernelGGL(k_entered_marks, dim3(rgrid), dim3(128), 0, s, d_reads, n_rec, fl, cx->mark.as<int>());
    if ((rc = rs.scan(s, cx->mark.as<int>(), n_rec, cx->at.as<int>(), &fl->n_valid))) return rc;
    hipLaunchKernelGGL(k_entered_write, dim3(rgrid), dim3(128), 0, s, cx->mark.as<int>(), cx->at.as<int>(), n_rec, d_rid);
    hipLaunchKernelGGL(k_hp_class, dim3(rgrid), dim3(128), 0, s, lin, d_reads, d_rid, fl, cx->hp.as<uint8_t>());
    hipLaunchKernelGGL(k_name_len, dim3(rgrid), dim3(128), 0, s, lin, d_reads, d_rid, fl, n_rec, cx->nlen.as<int>());
    if ((rc = rs.scan(s, cx->nlen.as<int>(), n_rec, cx->noff.as<int>(), reinterpret_cast<int*>(d_tot + 2)))) return rc;
    if (pr.max_depth > 0) hipLaunchKernelGGL(k_live, dim3(wgrid), dim3(256), 0, s, d_reads, d_rid, fl, pr.max_depth);
    CTO_HIP(hipEventRecord(cx->t[2], s));
    // ---- count pass, offsets ----
    CTO_HIP(hipMemsetAsync(cx->cnt.p, 0, size_t(n_col) * 4, s));
    CTO_HIP(hipMemsetAsync(cx->ibytes.p, 0, size_t(n_col) * 4, s));
    CTO_HIP(hipMemsetAsync(cx->cursor.p, 0, size_t(n_col) * 4, s));
    CTO_HIP(hipMemsetAsync(cx->flag.p, 0, size_t(n_col), s));
    hipLaunchKernelGGL(k_walk<false>, dim3(wgrid), dim3(256), 0, s, lin, d_reads, d_rid, fl, iv, pr.min_bq, pr.reverse_del, cx->cnt.as<int>(),
                       cx->ibytes.as<int>(), cx->flag.as<uint8_t>(), static_cast<const long long*>(nullptr), static_cast<int*>(nullptr),
                       static_cast<DRec*>(nullptr));
    if ((rc = rs.scan(s, cx->cnt.as<int>(), n_col, cx->col_off.as<long long>(), d_tot))) return rc;
    if ((rc = rs.scan(s, cx->ibytes.as<int>(), n_col, cx->ind_off.as<long long>(), d_tot + 1))) return rc;
    CTO_HIP(hipGetLastError());
    CTO_HIP(hipMemcpyAsync(cx->h_tot.p, d_tot, 24, hipMemcpyDeviceToHost, s));
    if ((rc = rs.fetch_flags(s))) return rc;
    if (hf->err_idx < hf->stop_idx) { *outcome = CHUNK_DAMAGED; return CTO_OK; }
    if (pr.max_depth > 0 && hf->deep_col) { *outcome = CHUNK_CAP; return CTO_OK; }
    const int n_valid = hf->n_valid;
    const long long n_recs = cx->h_tot.as<long long>()[0], n_ind = cx->h_tot.as<long long>()[1];
    const int n_name = *reinterpret_cast<const int*>(cx->h_tot.as<long long>() + 2);
    if (n_recs >= (1ll << 30) || n_ind >= (1ll << 31) - 1) { *outcome = CHUNK_TOO_LARGE; return CTO_OK; }
    // ---- fill pass, order, names; everything comes down once ----
    const size_t o_cnt = 0, o_flag = align16(o_cnt + size_t(n_col) * 4), o_recs = align16(o_flag + size_t(n_col)),
                 o_blob = align16(o_recs + size_t(n_recs) * sizeof(DRec)), o_noff = align16(o_blob + size_t(n_ind)),
                 o_names = align16(o_noff + size_t(n_valid + 1) * 4), o_hp = align16(o_names + size_t(n_name)), o_end = o_hp + size_t(n_valid);
    if ((rc = cx->tmp.ensure(size_t(n_recs + 1) * sizeof(DRec))) || (rc = cx->out.ensure(size_t(n_recs + 1) * sizeof(DRec))) ||
        (rc = cx->blob.ensure(size_t(n_ind) + 16)) || (rc = cx->names.ensure(size_t(n_name) + 16)) || (rc = cx->h_down.ensure(o_end + 16)))
        return rc;
    if (n_recs > 0) {
        hipLaunchKernelGGL(k_walk<true>, dim3(wgrid), dim3(256), 0, s, lin, d_reads, d_rid, fl, iv, pr.min_bq, pr.reverse_del, static_cast<int*>(nullptr),
                           static_cast<int*>(nullptr), static_cast<uint8_t*>(nullptr), cx->col_off.as<long long>(), cx->cursor.as<int>(),
                           cx->tmp.as<DRec>());
        hipLaunchKernelGGL(k_order, dim3(unsigned(std::min(n_col, 16384))), dim3(64), 0, s, lin, d_reads, d_rid, cx->cnt.as<int>(),
                           cx->col_off.as<long long>(), cx->ind_off.as<long long>(), n_col, cx->tmp.as<DRec>(), cx->out.as<DRec>(), cx->blob.as<char>());
    }
    if (n_valid > 0)
        hipLaunchKernelGGL(k_name_copy, dim3(unsigned(cdiv(n_valid, 128))), dim3(128), 0, s, lin, d_reads, d_rid, fl, cx->noff.as<int>(), cx->names.as<char>());
    CTO_HIP(hipGetLastError());
    CTO_HIP(hipEventRecord(cx->t[3], s));
    char* const h = cx->h_down.as<char>();
    CTO_HIP(hipMemcpyAsync(h + o_cnt, cx->cnt.p, size_t(n_col) * 4, hipMemcpyDeviceToHost, s));
    CTO_HIP(hipMemcpyAsync(h + o_flag, cx->flag.p, size_t(n_col), hipMemcpyDeviceToHost, s));
    if (n_recs > 0) CTO_HIP(hipMemcpyAsync(h + o_recs, cx->out.p, size_t(n_recs) * sizeof(DRec), hipMemcpyDeviceToHost, s));
    if (n_ind > 0) CTO_HIP(hipMemcpyAsync(h + o_blob, cx->blob.p, size_t(n_ind), hipMemcpyDeviceToHost, s));
    if (n_valid > 0) {
        CTO_HIP(hipMemcpyAsync(h + o_noff, cx->noff.p, size_t(n_valid + 1) * 4, hipMemcpyDeviceToHost, s));
        if (n_name > 0) CTO_HIP(hipMemcpyAsync(h + o_names, cx->names.p, size_t(n_name), hipMemcpyDeviceToHost, s));
        CTO_HIP(hipMemcpyAsync(h + o_hp, cx->hp.p, size_t(n_valid), hipMemcpyDeviceToHost, s));
    }
    CTO_HIP(hipEventRecord(cx->t[4], s));
    if ((rc = rs.wait(s))) return rc;
    st->n_reads_entered += n_valid;
    float ms = 0.f;
    CTO_HIP(hipEventElapsedTime(&ms, cx->t[0], cx->t[1])); st->ms_inflate += ms;
    CTO_HIP(hipEventElapsedTime(&ms, cx->t[1], cx->t[2])); st->ms_records += ms;
    CTO_HIP(hipEventElapsedTime(&ms, cx->t[2], cx->t[3])); st->ms_kernels += ms;
    CTO_HIP(hipEventElapsedTime(&ms, cx->t[3], cx->t[4])); st->ms_down += ms;
    // ---- the chunk's raw columns ----
    const double tb0 = now_ms();
    const int* h_cnt = reinterpret_cast<const int*>(h + o_cnt);
    const uint8_t* h_flag = reinterpret_cast<const uint8_t*>(h + o_flag);
    const HapRawRec* h_recs = reinterpret_cast<const HapRawRec*>(h + o_recs);
    const int* h_noff = reinterpret_cast<const int*>(h + o_noff);
    raw->names.resize(size_t(n_valid));
    for (int j = 0; j < n_valid; ++j) raw->names[size_t(j)].assign(h + o_names + h_noff[j], size_t(h_noff[j + 1] - h_noff[j]));
    raw->hp.assign(h + o_hp, h + o_hp + n_valid);
    raw->indel.assign(h + o_blob, size_t(n_ind));
    int64_t at = 0;
    for (size_t i = 0; i < np; ++i)
        for (int64_t p = pc[a + i].s; p < pc[a + i].e; ++p) {
            const int c = iv_base[i] + int(p - pc[a + i].s);
            const int64_t nc = h_cnt[c];
            if (h_flag[c]) skipped->push_back(p);
            else if (nc > 0) {
                raw->recs.insert(raw->recs.end(), h_recs + at, h_recs + at + nc);
                hap_rse_from_marks(h_recs + at, nc, &raw->rse);
                raw->col_pos.push_back(p + 1);
                raw->col_off.push_back(int64_t(raw->recs.size()));
                raw->rse_off.push_back(int64_t(raw->rse.size()));
            }
            at += nc;
        }
    st->ms_build += now_ms() - tb0;
    return CTO_OK;
}

int64_t chunk_budget() {
    if (const char* e = getenv("CTO_HAP_CHUNK_BYTES")) { const long long v = atoll(e); if (v > 0) return v; }
    return int64_t(256) << 20;
}

// raw's columns and the host's (rebuilt) columns into the job, in ascending position
int add_merged(void* job, const HapRaw& dev, const HapRaw& host) {
    size_t i = 0, j = 0;
    const size_t ni = dev.col_pos.size(), nj = host.col_pos.size();
    int rc;
    while (i < ni || j < nj) {
        if (j == nj || (i < ni && dev.col_pos[i] < host.col_pos[j])) {
            size_t e = i + 1;
            while (e < ni && (j == nj || dev.col_pos[e] < host.col_pos[j])) ++e;
            if ((rc = hap_job_add(job, dev, int64_t(i), int64_t(e)))) return rc;
            i = e;
        } else {
            size_t e = j + 1;
            while (e < nj && (i == ni || host.col_pos[e] < dev.col_pos[i])) ++e;
            if ((rc = hap_job_add(job, host, int64_t(j), int64_t(e)))) return rc;
            j = e;
        }
    }
    return CTO_OK;
}

}  // namespace

extern "C" int cto_hap_windows(const char* bam_path, const char* bai_path, const char* ctg_name, int64_t region_lo, int64_t region_hi,
                               const int64_t* iv, int64_t n_iv, int min_mq, int min_bq, int excl_flags, int max_depth, int reverse_del, int where,
                               void** job_out, cto_hap_stats* stats) {
    void* job = nullptr;
    const int rc = guarded("cto_hap_windows", [&]() -> int {
        CTO_REQUIRE(bam_path && ctg_name && job_out && (iv || n_iv == 0) && n_iv >= 0, CTO_EINVAL, "cto_hap_windows: null argument");
        CTO_REQUIRE(where == 0 || where == 1, CTO_EINVAL, "cto_hap_windows: where must be 0 (host) or 1 (device)");
        CTO_REQUIRE(region_lo >= 1 && region_hi >= region_lo && region_hi < INT32_MAX, CTO_EINVAL, "cto_hap_windows: bad region %lld-%lld",
                    (long long)region_lo, (long long)region_hi);
        CTO_REQUIRE(max_depth >= 0 && min_bq >= 0, CTO_EINVAL, "cto_hap_windows: max_depth and min_bq must not be negative");
        *job_out = nullptr;
        cto_hap_stats st{};
        if (stats) *stats = st;
        int rc;
        if ((rc = hap_job_new(region_lo, region_hi, &job))) return rc;
        // the wanted positions: the intervals clipped to the region (all of it without them), in pieces of at most 4 kb
        std::vector<Piece> pc;
        auto add_pieces = [&](int64_t s, int64_t e) {
            s = std::max(s, region_lo - 1);
            e = std::min(e, region_hi);
            for (; s < e; s += 4096) pc.push_back(Piece{s, std::min(e, s + 4096)});
        };
        if (!iv) add_pieces(region_lo - 1, region_hi);
        for (int64_t k = 0; iv && k < n_iv; ++k) {
            CTO_REQUIRE(iv[2 * k] >= 0 && iv[2 * k + 1] >= iv[2 * k] && (k == 0 || iv[2 * k] >= iv[2 * k - 1]), CTO_EINVAL,
                        "cto_hap_windows: intervals must be 0-based [s, e), ascending and disjoint");
            add_pieces(iv[2 * k], iv[2 * k + 1]);
        }
        const HapWinParams pr{min_mq, min_bq, excl_flags, max_depth, reverse_del != 0};
        HapRaw raw, raw_host;
        std::vector<int64_t> flat;
        auto on_host = [&](size_t a, size_t b) -> int {             // pieces [a, b) by the host rules, into the job
            flat.clear();
            for (size_t i = a; i < b; ++i) { flat.push_back(pc[i].s); flat.push_back(pc[i].e); }
            raw.clear();
            int64_t entered = 0;
            int r = hap_windows_host(bam_path, bai_path, ctg_name, region_lo, region_hi, flat.data(), int64_t(b - a), pr, &raw, &entered);
            if (r != CTO_OK) return r;
            st.n_reads_entered += entered;
            const double tb0 = now_ms();
            r = hap_job_add(job, raw, 0, int64_t(raw.col_pos.size()));
            st.ms_build += now_ms() - tb0;
            return r;
        };
        if (pc.empty()) { *job_out = job; job = nullptr; return CTO_OK; }
        if (where == 0) {
            if ((rc = on_host(0, pc.size()))) return rc;
            st.n_chunks = 1;
        } else {
            std::vector<int32_t> loci(pc.size());
            for (size_t i = 0; i < pc.size(); ++i) loci[i] = int32_t(pc[i].s + 1);
            std::vector<int64_t> cuts;
            if ((rc = allele_plan_chunks(bam_path, bai_path, ctg_name, loci.data(), int64_t(loci.size()), chunk_budget(), &cuts))) return rc;
            HwCtx& cx = process_wide<HwCtx>();
            std::lock_guard<std::mutex> lock(cx.mu);
            for (Event& e : cx.t) if (!e && (rc = e.create())) return rc;
            hipStream_t s = nullptr;
            std::vector<std::pair<size_t, size_t>> todo;            // a stack: a chunk found too large is halved
            for (size_t c = cuts.size() - 1; c-- > 0;) todo.push_back({size_t(cuts[c]), size_t(cuts[c + 1])});
            std::vector<int64_t> skipped;
            while (!todo.empty()) {
                const auto [a, b] = todo.back();
                todo.pop_back();
                int outcome = CHUNK_DONE;
                raw.clear();
                skipped.clear();
                if (pr.max_depth > 0 && a > 0) outcome = CHUNK_CAP;     // the cap looks at every read from the region's start
                else if ((rc = windows_chunk_device(&cx, bam_path, bai_path, ctg_name, pc, a, b, pr.max_depth > 0 ? region_lo : pc[a].s + 1, pr, s,
                                                    &st, &raw, &skipped, &outcome)))
                    return rc;
                if (outcome == CHUNK_TOO_LARGE) {
                    if (b - a > 1) {
                        todo.push_back({a + (b - a) / 2, b});
                        todo.push_back({a, a + (b - a) / 2});
                        continue;
                    }
                    outcome = CHUNK_DAMAGED;                         // 4 kb of positions past the device's offsets: the host's
                }
                ++st.n_chunks;
                if (outcome != CHUNK_DONE) {
                    if ((rc = on_host(a, b))) return rc;
                    st.fallback_chunks += outcome == CHUNK_DAMAGED;
                    st.cap_chunks += outcome == CHUNK_CAP;
                    continue;
                }
                // the columns a printing skip covers, by the host rule: runs of neighbours as intervals
                raw_host.clear();
                if (!skipped.empty()) {
                    flat.clear();
                    for (const int64_t p : skipped) {
                        if (!flat.empty() && flat.back() == p) flat.back() = p + 1;
                        else { flat.push_back(p); flat.push_back(p + 1); }
                    }
                    if ((rc = hap_windows_host(bam_path, bai_path, ctg_name, region_lo, region_hi, flat.data(), int64_t(flat.size() / 2), pr, &raw_host,
                                               nullptr)))
                        return rc;
                    st.host_columns += int64_t(skipped.size());
                }
                const double tb0 = now_ms();
                if ((rc = add_merged(job, raw, raw_host))) return rc;
                st.ms_build += now_ms() - tb0;
            }
        }
        cto_hap_view v;
        if ((rc = cto_hap_job_view(job, &v))) return rc;
        st.n_cols = v.n_cols;
        st.n_recs = v.n_recs;
        if (stats) *stats = st;
        *job_out = job;
        job = nullptr;
        return CTO_OK;
    });
    if (job) cto_hap_job_free(job);
    return rc;
}
