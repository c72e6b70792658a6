// Reads -> columns on the device (BASELINE.json north_star: "stages per-site read pileups ... on the GPU"):
// the column pack of cto_pack_from_bam, built in HBM from BGZF blocks that csrc/inflate.hip inflated there - the alignment
// records never travel back to the host and no pack travels up.
//
// PARITY UNPINNED against samtools (absent from both boxes), like the host reader it restates (csrc/bam.cpp: the pileup rules are
// listed in its header).  What IS held: every array of the pack equal to cto_pack_from_bam's, bit for bit, on every BAM the test
// suite writes (tests/test_gpu_pileup.py) - the host reader is the specification of this file.
//
// Pipeline (one chunk = one call, all kernels on the caller's stream; the first three are bam_records.h's, queued by its RecordStream):
//   k_linearise     the inflated blocks (256-byte aligned output slots) -> one contiguous record stream
//   k_chain         record boundaries: every virtual offset the .bai names (chunk starts, the linear index's 16 kb windows) is the
//                   head of a chain of `block_size` hops walked by one lane; counted, then written in file order
//   k_parse         one lane per record: header filters (reference id, excluded flags, MAPQ, orphan), CIGAR lengths (CG:B,I for
//                   > 65535 operations), the region test; the first record that ends the region's scan cuts the list
//   k_compact       accepted reads in file order
//   k_cover         +1 / -1 per read at the first / one-past-last REQUESTED position it covers (the BED intervals of the
//                   candidate windows, concatenated: a read covers a contiguous run of that space)
//   k_columns_*     running sum -> depth per requested position, rows only where depth > 0, entry offsets (tile sums, their scan
//                   by one workgroup, then every 4096-position tile on top of its base)
//   k_fill          one wave per read, one lane per CIGAR operation (prefix sums over 64 operations at a time give every lane
//                   its reference / query offsets): read-bases, deletion placeholders and the indel attached to the last base
//                   of an aligned run go straight to their place in their column - file order = the number of earlier reads
//                   that cover the position, counted against the ends of the reads still open at this read's start
//   k_order         one wave per column that holds an indel carrier: the distinct indel keys in first-seen order (candidates
//                   compared against the column's keys across lanes), merged candidate-extraction groups
//   k_keys_*        key tables and the alt_info key strings ("I<ANCHOR><SEQ>", "D<reference slice>")
// Two round trips to the host are needed (sizes for allocation): after k_columns and after the per-column key counts.
//
// Not done here - the call reports `fallback` and the caller uses the host reader: paired reads (mate-overlap quality edits are
// order dependent), reference skips (N), --max-depth or more reads open at some read's start (the cap is order dependent; k_live_marks), a column
// deeper than 2048, 2048 or more reads open at a read's start, or more than 64 distinct indel keys in a column.  The BGZF CRC-32 of every block is
// checked on the device (k_crc32_blocks), as htslib and the host reader check it.
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "bam_records.h"
#include "common.h"
#include "hip_buffers.h"
#include "pack_internal.h"
#include "scan.h"

using namespace cto;

namespace {

struct TmpEnt { uint32_t entry, rank, ind_q, ind; };      // ind = len << 2 | kind (0 none, 1 ins, 2 del)
struct KeyRec { uint32_t read, q, len; uint8_t code, kind, overlong, group; };

// accepted reads (in front of the record that ended the scan) in file order: rid[j] = record index
__global__ void k_compact(const DevRead* __restrict__ reads, int n_rec, int* __restrict__ rid, Flags* fl) {
    __shared__ int part[1024];
    const int stop = fl->stop_idx;
    const int n = min(n_rec, stop), t = threadIdx.x, per = (n + blockDim.x - 1) / blockDim.x;
    const int lo = min(n, t * per), hi = min(n, lo + per);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += reads[i].valid;
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < int(blockDim.x); d <<= 1) {
        const int v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = part[t] - s, longest = 0;
    for (int i = lo; i < hi; ++i) if (reads[i].valid) { rid[run++] = i; longest = max(longest, reads[i].end - reads[i].pos); }
    if (longest > 0) atomicMax(&fl->max_len, longest);
    if (t == int(blockDim.x) - 1) fl->n_valid = part[t];
}

// The --max-depth cap (host reader, csrc/bam.cpp: a read is dropped when max_depth accepted reads are still open at its start) can
// only bite where that many reads overlap a read's start.  Accepted reads are in file order = sorted by start, so read j is open at
// the start of exactly the reads j+1 .. nxt(j)-1, nxt(j) = the first later read starting at or behind j's end: +1 / -1 marks over the
// read index, a running sum, its maximum.  Below max_depth no read is dropped and the device pack is the host's; otherwise fallback.
__global__ void k_live_marks(const DevRead* __restrict__ reads, const int* __restrict__ rid, const Flags* fl, int* __restrict__ marks) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x, n = fl->n_valid;
    if (j >= n) return;
    const int end = reads[rid[j]].end;
    int a = j + 1, b = n;
    while (a < b) { const int m = (a + b) >> 1; if (reads[rid[m]].pos >= end) b = m; else a = m + 1; }
    if (a > j + 1) { atomicAdd(&marks[j + 1], 1); atomicAdd(&marks[a], -1); }
}
__global__ void k_live_max(const int* __restrict__ marks, Flags* fl) {       // one workgroup
    __shared__ int part[1024], best[1024];
    const int n = fl->n_valid + 1, t = threadIdx.x, per = (n + blockDim.x - 1) / blockDim.x;
    const int lo = min(n, t * per), hi = min(n, lo + per);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += marks[i];
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < int(blockDim.x); d <<= 1) {
        const int v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = part[t] - s, m = 0;
    for (int i = lo; i < hi; ++i) { run += marks[i]; m = max(m, run); }
    best[t] = m;
    __syncthreads();
    for (int d = int(blockDim.x) >> 1; d > 0; d >>= 1) {
        if (t < d) best[t] = max(best[t], best[t + d]);
        __syncthreads();
    }
    if (t == 0) fl->max_live = best[0];
}

// Requested positions: n_iv sorted, disjoint 0-based intervals [lo, hi) clipped to the region; slot space = their concatenation
struct Ivs { const int* lo; const int* hi; const int* base; int n; int total; };
__device__ __forceinline__ int first_slot_ge(const Ivs& v, int p) {    // slot of the first requested position >= p (total: none)
    int a = 0, b = v.n;
    while (a < b) { const int m = (a + b) >> 1; if (v.hi[m] > p) b = m; else a = m + 1; }
    if (a >= v.n) return v.total;
    return v.base[a] + (p > v.lo[a] ? p - v.lo[a] : 0);
}

__global__ void k_cover(const DevRead* __restrict__ reads, const int* __restrict__ rid, const Flags* fl, Ivs iv, int* __restrict__ diff) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= fl->n_valid) return;
    const DevRead& r = reads[rid[j]];
    const int a = first_slot_ge(iv, r.pos), b = first_slot_ge(iv, r.end);
    if (b > a) { atomicAdd(&diff[a], 1); atomicAdd(&diff[b], -1); }
}

constexpr int ORD_DMAX_COLS = 2048;      // = ORD_DMAX of k_order
// One workgroup (1024 threads, 4096 slots per pass, coalesced): depth per slot (running sum of diff), rows where depth > 0
// (slot_col, col_slot), col_off.
// k_columns over the chip: (1) tile sums of the marks, scanned -> the depth in front of every tile; (2) per tile the number of
// positions with depth > 0 and the sum of their depths, scanned -> the first column / entry of every tile; (3) every tile writes
// its rows.  The one-workgroup form took 3.7 ms for the million positions of a region piled up without a BED.
__device__ __forceinline__ void tile_depths(const int* __restrict__ diff, int total, long long before, int i0, long long* wsum, int (&d)[4],
                                            long long (&dep)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = i0 + k < total ? diff[i0 + k] : 0;
    long long tot;
    long long depth = before + block_scan_excl((long long)d[0] + d[1] + d[2] + d[3], &tot, wsum);
#pragma unroll
    for (int k = 0; k < 4; ++k) { depth += d[k]; dep[k] = i0 + k < total ? depth : 0; }
}
__global__ __launch_bounds__(1024) void k_columns_count(const int* __restrict__ diff, int total, const long long* __restrict__ depth_base,
                                                        long long* __restrict__ tcnt /* [tiles][2] */) {
    __shared__ long long wsum[17];
    const int i0 = blockIdx.x * SCAN_TILE + 4 * threadIdx.x;
    int d[4];
    long long dep[4];
    tile_depths(diff, total, depth_base[blockIdx.x], i0, wsum, d, dep);
    long long nz = 0, ds = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { nz += dep[k] > 0; ds += dep[k]; }
    long long tn, td;
    (void)block_scan_excl(nz, &tn, wsum);
    (void)block_scan_excl(ds, &td, wsum);
    if (threadIdx.x == 0) { tcnt[size_t(blockIdx.x) * 2] = tn; tcnt[size_t(blockIdx.x) * 2 + 1] = td; }
}
__global__ __launch_bounds__(1024) void k_columns_write(const int* __restrict__ diff, int total, const long long* __restrict__ depth_base,
                                                        const long long* __restrict__ tcnt, const long long* __restrict__ totals,
                                                        int* __restrict__ slot_col, int* __restrict__ col_slot, long long* __restrict__ col_off, Flags* fl) {
    __shared__ long long wsum[17];
    const int i0 = blockIdx.x * SCAN_TILE + 4 * threadIdx.x;
    int d[4];
    long long dep[4];
    tile_depths(diff, total, depth_base[blockIdx.x], i0, wsum, d, dep);
    long long nz = 0, ds = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { nz += dep[k] > 0; ds += dep[k]; }
    long long tn, td;
    long long c = tcnt[size_t(blockIdx.x) * 2] + block_scan_excl(nz, &tn, wsum);
    long long o = tcnt[size_t(blockIdx.x) * 2 + 1] + block_scan_excl(ds, &td, wsum);
    bool deep = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (i0 + k >= total) break;
        if (dep[k] > 0) { slot_col[i0 + k] = int(c); col_slot[c] = i0 + k; col_off[c] = o; ++c; o += dep[k]; deep |= dep[k] > ORD_DMAX_COLS; }
        else slot_col[i0 + k] = -1;
    }
    if (deep) atomicExch(&fl->deep_col, 1);
    if (blockIdx.x == 0 && threadIdx.x == 0) { fl->n_cols = int(totals[0]); fl->n_entries = totals[1]; col_off[totals[0]] = totals[1]; }
}

__global__ void k_col_meta(const int* __restrict__ col_slot, int n_cols, Ivs iv, const char* __restrict__ ref, long long ref_start, long long ref_len,
                           int32_t* __restrict__ col_pos, uint8_t* __restrict__ col_ref, Flags* fl) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cols) return;
    const int s = col_slot[c];
    int a = 0, b = iv.n;
    while (b - a > 1) { const int m = (a + b) >> 1; if (iv.base[m] <= s) a = m; else b = m; }
    const long long pos1 = (long long)iv.lo[a] + (s - iv.base[a]) + 1, ri = pos1 - ref_start;
    col_pos[c] = int32_t(pos1);
    if (ri < 0 || ri >= ref_len) { atomicExch(&fl->ref_oob, 1); col_ref[c] = 0; return; }
    char ch = ref[ri];
    if (ch >= 'a' && ch <= 'z') ch = char(ch - 32);
    const int code = ch == 'C' ? 1 : (ch == 'G' ? 2 : (ch == 'T' ? 3 : 0));
    const bool acgt = ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T';
    col_ref[c] = uint8_t(code | (acgt ? 0 : 0x80));
}

__device__ __forceinline__ uint32_t dev_entry(int code, int bq, int mq) { return uint32_t(code) | (uint32_t(bq) << 6) | (uint32_t(mq) << 13); }
__constant__ int8_t kNib[16] = {-1, 0, 1, 10, 2, 10, 10, 10, 3, 10, 10, 10, 10, 10, 10, 10};

// One wave per accepted read, one lane per CIGAR operation (64 at a time).
// Where an entry goes (round 4): a column lists its reads in file order, and read j's place in the column of position p is the number
// of EARLIER reads that cover p - all of which started at or before j's start (the file is sorted), so they are the reads still open
// at j's start whose end lies behind p.  The wave collects the ends of those open reads once (the accepted reads in front of j, back
// to the first one that starts more than the longest read's span before j) and counts, per position, the ends behind it: no cursor
// atomics (device-scope atomics from eight XCDs on 51 M read-bases were most of this kernel's time), no rank to carry along, nothing
// to put back into order afterwards - the 4-byte entry lands in its final place.  Indel carriers (one read-base in a hundred) leave
// their details in `side` at the same index and a mark on their column for k_order.
constexpr int FILL_LIVE_MAX = 2048;          // reads open at a read's start the kernel can hold (more: the caller falls back)
__global__ __launch_bounds__(256) void k_fill(int live_cap, const uint8_t* __restrict__ lin, const DevRead* __restrict__ reads, const int* __restrict__ rid,
                                              Flags* fl, Ivs iv, const int* __restrict__ slot_col, const long long* __restrict__ col_off,
                                              int* __restrict__ marks, uint32_t* __restrict__ entries, TmpEnt* __restrict__ side,
                                              const char* __restrict__ ref, long long ref_start, long long ref_len) {
    // [wave][live_cap] ends as collected, then [wave][live_cap] sorted; live_cap = the launch's bound on reads open at a read's start
    // (k_live_max), so that ordinary depths leave the LDS - and with it the number of reads in flight per CU - alone
    extern __shared__ int s_fill[];
    int* const s_live_w = s_fill + (threadIdx.x >> 6) * live_cap;
    int* const s_sort_w = s_fill + (4 + (threadIdx.x >> 6)) * live_cap;
    // The four waves of a workgroup share ONE read (each walks the CIGAR for itself and takes every fourth 64-position slice of a long
    // run, every fourth short operation): the kernel lasts as long as its longest read's chain of dependent trips to memory
    // (position -> column -> entry offset -> store, ~3 us a slice), and a 30 kb read is 470 slices.
    // Workgroups are dealt to the 8 XCDs in turn: XCD x takes the x-th eighth of the (position-sorted) reads, so that the reads an XCD
    // works on at one time lie next to each other on the genome and their four-byte stores - every one to another cache line of the
    // column-major entries - meet again in that XCD's own L2 before the lines go to memory
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int per_xcd = (fl->n_valid + 7) >> 3;
    const int j = int(blockIdx.x & 7u) * per_xcd + int(blockIdx.x >> 3);
    if (int(blockIdx.x >> 3) >= per_xcd || j >= fl->n_valid) return;
    const DevRead r = reads[rid[j]];
    int n_live = 0;
    {
        const long long reach = (long long)r.pos - fl->max_len;       // a read that starts at or before it has ended by r.pos
        for (int i0 = j - 1; i0 >= 0; i0 -= 64) {
            const int i = i0 - lane;
            int ps = 0, en = 0;
            if (i >= 0) { const int ri = rid[i]; ps = reads[ri].pos; en = reads[ri].end; }
            const bool open = i >= 0 && en > r.pos;
            const unsigned long long m = __ballot(open);
            const int at = n_live + __popcll(m & ((1ull << lane) - 1ull));
            if (open && at < live_cap) s_live_w[at] = en;
            n_live += __popcll(m);
            if (__ballot(i >= 0 && (long long)ps <= reach)) break;
        }
        if (n_live > live_cap) { if (lane == 0) atomicExch(&fl->deep_col, 1); return; }      // cannot happen (live_cap > max_live); the caller falls back
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_wave_barrier();
        // ascending (rank by counting; n_live is about the depth): a position's count is then a binary search, not a sweep
        for (int u0 = 0; u0 < n_live; u0 += 64) {
            const int idx = u0 + lane;
            const int v = idx < n_live ? s_live_w[idx] : 0x7fffffff;
            int rk = 0;
            for (int k = 0; k < n_live; ++k) { const int x = s_live_w[k]; rk += (x < v) || (x == v && k < idx); }
            if (idx < n_live) s_sort_w[rk] = v;
        }
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_wave_barrier();
    }
    const int* const live = s_sort_w;
    const uint8_t* ops = lin + r.ops_off;
    const uint8_t* seq = lin + r.seq_off;
    const uint8_t* qual = lin + r.qual_off;
    const int mq = min(int(r.mapq), 93);
    auto base4 = [&](int q) { return (seq[q >> 1] >> ((~q & 1) << 2)) & 15; };
    auto bq = [&](int q) { return (r.no_qual || q >= r.l_seq) ? 0 : min(int(qual[q]), 93); };
    int ref_carry = r.pos, q_carry = 0;
    for (int k0 = 0; k0 < r.n_ops; k0 += 64) {
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
        const bool covers = k < r.n_ops && cons_ref && opc != 3;
        const bool aligned = opc != 2;
        // the indel that follows this aligned run (P operations skipped)
        uint32_t ind = 0, ind_q = 0;
        if (covers && aligned) {
            int nx = k + 1;
            while (nx < r.n_ops && (ld32(ops + size_t(nx) * 4) & 15) == 6) ++nx;
            if (nx < r.n_ops) {
                const uint32_t nc = ld32(ops + size_t(nx) * 4);
                const int nop = int(nc & 15), nlen = int(nc >> 4);
                if (nop == 1) { ind = (uint32_t(nlen) << 2) | 1u; ind_q = uint32_t(op_q + len); }
                else if (nop == 2) ind = (uint32_t(nlen) << 2) | 2u;
            }
        }
        // the read's contribution at reference position p of the operation (o_ref, o_q, o_len, ...)
        // the entry of reference position p and its column; the trip to the column's cursor is the caller's (several in flight)
        auto make = [&](int p, int kiv, int o_ref, int o_q, int o_len, bool o_aligned, uint32_t o_ind, uint32_t o_ind_q, TmpEnt* out) -> int {
            const int col = slot_col[iv.base[kiv] + (p - iv.lo[kiv])];
            TmpEnt e;
            e.rank = uint32_t(j);
            e.ind = 0;
            e.ind_q = 0;
            if (!o_aligned) {
                e.entry = dev_entry(r.rev ? 9 : 8, bq(o_q), mq);
            } else {
                const int q = o_q + (p - o_ref);
                int code = kNib[base4(q)];
                if (code < 0) {
                    const long long ri = (long long)p + 1 - ref_start;
                    char ch = (ri >= 0 && ri < ref_len) ? ref[ri] : 'N';
                    if (ch >= 'a' && ch <= 'z') ch = char(ch - 32);
                    code = ch == 'A' ? 0 : (ch == 'C' ? 1 : (ch == 'G' ? 2 : (ch == 'T' ? 3 : 10)));
                }
                if (r.rev) code += code < 4 ? 4 : 1;
                e.entry = dev_entry(code, bq(q), mq);
                if (p == o_ref + o_len - 1) { e.ind = o_ind; e.ind_q = o_ind_q; }
            }
            *out = e;
            return col;
        };
        auto emit = [&](int p, int kiv, int o_ref, int o_q, int o_len, bool o_aligned, uint32_t o_ind, uint32_t o_ind_q) {
            TmpEnt e;
            const int col = make(p, kiv, o_ref, o_q, o_len, o_aligned, o_ind, o_ind_q, &e);
            int lo = 0, n = n_live;                                             // first end behind p: the earlier reads that cover p
            while (n > 0) {
                const int half = n >> 1;
                if (live[lo + half] <= p) { lo += half + 1; n -= half + 1; } else n = half;
            }
            const long long at = col_off[col] + (n_live - lo);
            entries[at] = e.entry | ((e.ind & 3u) << 4);                        // carriers: provisional kind, k_order completes it
            if (e.ind & 3u) { side[at] = e; marks[col] = 1; }
        };
        auto first_iv = [&](int p) {
            int a = 0, b = iv.n;
            while (a < b) { const int m = (a + b) >> 1; if (iv.hi[m] > p) b = m; else a = m + 1; }
            return a;
        };
        // short operations (real long-read CIGARs: an indel every ~10-20 bases): the lane walks its own; long aligned runs
        // (hundreds of bases) would leave the other lanes idle, so the whole wave takes each of those in turn below
        constexpr int LONG_OP = 48;
        const bool is_long = covers && len > LONG_OP;
        if (covers && !is_long && (k & 3) == wv) {
            int p = op_ref, kiv = first_iv(op_ref);
            const int pend = op_ref + len;
            while (p < pend && kiv < iv.n) {
                if (p < iv.lo[kiv]) { p = iv.lo[kiv]; continue; }
                if (p >= iv.hi[kiv]) { ++kiv; continue; }
                const int stop = min(pend, iv.hi[kiv]);
                for (; p < stop; ++p) emit(p, kiv, op_ref, op_q, len, aligned, ind, ind_q);
            }
        }
        unsigned long long lm = __ballot(is_long);
        while (lm) {
            const int src = __ffsll((long long)lm) - 1;
            lm &= lm - 1;
            const int o_ref = __shfl(op_ref, src), o_q = __shfl(op_q, src), o_len = __shfl(len, src);
            const bool o_aligned = __shfl(int(aligned), src) != 0;
            const uint32_t o_ind = __shfl(ind, src), o_ind_q = __shfl(ind_q, src);
            const int pend = o_ref + o_len;
            for (int kiv = first_iv(o_ref); kiv < iv.n && iv.lo[kiv] < pend; ++kiv) {
                const int lo = max(o_ref, iv.lo[kiv]), hi = min(pend, iv.hi[kiv]);
                if (hi - lo > 64) {              // a long stretch of requested positions: every wave takes each fourth 64-position slice
                    for (int p = lo + lane + 64 * wv; p < hi; p += 256) emit(p, kiv, o_ref, o_q, o_len, o_aligned, o_ind, o_ind_q);
                } else if ((kiv & 3) == wv) {    // candidate windows (34 positions each): every wave takes each fourth window
                    const int p = lo + lane;
                    if (p < hi) emit(p, kiv, o_ref, o_q, o_len, o_aligned, o_ind, o_ind_q);
                }
            }
        }
    }
}

constexpr int ORD_KMAX = 64;

__device__ __forceinline__ int canon_nib(const uint8_t* seq, int q) {
    const int n = (seq[q >> 1] >> ((~q & 1) << 2)) & 15;
    return n == 0 ? 15 : n;                       // '=' prints as N, like nibble 15
}

struct IndEnt { uint32_t at, entry, rank, ind_q, ind; };     // at = the entry's place in the column once it is in file order

// The indel keys of the columns k_fill marked (round 4: the entries are in file order already): one wave per marked column walks its
// entries 64 at a time, and every indel carrier - in file order - is compared against the column's keys across lanes: the distinct keys
// in first-seen order, the merged candidate-extraction groups, the entry completed with kind and key id.  Columns without a carrier
// (six in ten at 50x) cost one coalesced load of 64 marks per wave trip.
__global__ __launch_bounds__(64) void k_order(const uint8_t* __restrict__ lin, const DevRead* __restrict__ reads, const int* __restrict__ rid,
                                              int n_cols, const long long* __restrict__ col_off, const int* __restrict__ marks,
                                              const TmpEnt* __restrict__ side, uint32_t* __restrict__ entries, int* __restrict__ n_keys_col,
                                              KeyRec* __restrict__ keyrec, int max_indel, Flags* fl) {
    __shared__ KeyRec keys[ORD_KMAX];
    __shared__ int grp_key[ORD_KMAX];             // group g is represented by the key that opened it
    const int lane = threadIdx.x;
    for (long long base = blockIdx.x * 64ll; base < n_cols; base += gridDim.x * 64ll) {
        const long long cc = base + lane;
        const bool marked = cc < n_cols && marks[cc] != 0;
        if (cc < n_cols && !marked) n_keys_col[cc] = 0;
        unsigned long long todo = __ballot(marked);
        while (todo) {
            const int c = int(base) + __ffsll((long long)todo) - 1;
            todo &= todo - 1ull;
            const long long o = col_off[c];
            const int d = int(col_off[c + 1] - o);
            __syncthreads();
            int nk = 0, ng = 0;
            bool over = false;
            for (int i0 = 0; i0 < d && !over; i0 += 64) {
                const int i = i0 + lane;
                const uint32_t ent = i < d ? entries[o + i] : 0u;
                unsigned long long car = __ballot(i < d && ((ent >> 4) & 3u) != 0u);
                while (car && !over) {
                    const int src = __ffsll((long long)car) - 1;
                    car &= car - 1ull;
                    const int cat = i0 + src;
                    const TmpEnt cand = side[o + cat];                             // the same for every lane
                    const uint32_t centry = cand.entry;
                    const int kind = int(cand.ind & 3u), len = int(cand.ind >> 2), code = int(centry & 15u);
                    const uint8_t* cseq = lin + reads[rid[cand.rank]].seq_off;
                    bool hit = false;
                    if (lane < nk) {                                               // lane k compares the candidate with key k
                        const KeyRec kr = keys[lane];
                        if (int(kr.code) == code && int(kr.kind) == kind && int(kr.len) == len) {
                            hit = true;
                            if (kind == 1) {
                                const uint8_t* kseq = lin + reads[rid[kr.read]].seq_off;
                                for (int t = 0; t < len; ++t)
                                    if (canon_nib(kseq, int(kr.q) + t) != canon_nib(cseq, int(cand.ind_q) + t)) { hit = false; break; }
                            }
                        }
                    }
                    const unsigned long long hm = __ballot(hit);
                    int kid;
                    if (hm) {
                        kid = __ffsll((long long)hm) - 1;
                    } else {
                        if (nk >= ORD_KMAX) { over = true; break; }
                        kid = nk;
                        // merged group for candidate extraction: insertions by upper-cased anchor + sequence, deletions by length
                        const char anchor_c = "ACGTACGT*#NN"[code];
                        bool ghit = false;
                        if (lane < ng) {
                            const KeyRec gr = keys[grp_key[lane]];
                            if (int(gr.kind) == kind && int(gr.len) == len) {
                                if (kind == 2) ghit = true;
                                else if ("ACGTACGT*#NN"[gr.code] == anchor_c) {
                                    ghit = true;
                                    const uint8_t* gseq = lin + reads[rid[gr.read]].seq_off;
                                    for (int t = 0; t < len; ++t)
                                        if (canon_nib(gseq, int(gr.q) + t) != canon_nib(cseq, int(cand.ind_q) + t)) { ghit = false; break; }
                                }
                            }
                        }
                        const unsigned long long gm = __ballot(ghit);
                        const int g = gm ? __ffsll((long long)gm) - 1 : ng;
                        if (lane == 0) {
                            const int gate = kind == 1 ? len : len + 1;
                            keys[nk] = KeyRec{cand.rank, cand.ind_q, uint32_t(len), uint8_t(code), uint8_t(kind), uint8_t(gate > max_indel), uint8_t(g)};
                            if (!gm) grp_key[ng] = nk;
                        }
                        if (!gm) ++ng;
                        ++nk;
                        __syncthreads();
                    }
                    if (lane == 0) {
                        const int gate = kind == 1 ? len : len + 1;
                        entries[o + cat] = centry | (uint32_t(gate > max_indel ? 3 : kind) << 4) | (uint32_t(kid) << 21);
                    }
                }
            }
            if (over) { if (lane == 0) { atomicExch(&fl->many_keys, 1); n_keys_col[c] = 0; } continue; }
            __syncthreads();
            if (lane == 0) n_keys_col[c] = nk;
            for (int k = lane; k < nk; k += 64) keyrec[o + k] = keys[k];          // nk <= d: the column's own slots
        }
    }
}

// key tables in column order + the length of every alt_info key string
__global__ void k_keys_meta(int n_cols, const long long* __restrict__ col_off, const int* __restrict__ key_off, const KeyRec* __restrict__ keyrec,
                            const int32_t* __restrict__ col_pos, long long ref_start, long long ref_len, int max_indel, uint8_t* __restrict__ key_meta,
                            int32_t* __restrict__ key_group, KeyRec* __restrict__ key_final, int* __restrict__ key_col, int* __restrict__ key_len) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cols) return;
    const int k0 = key_off[c], nk = key_off[c + 1] - k0;
    for (int k = 0; k < nk; ++k) {
        const KeyRec kr = keyrec[col_off[c] + k];
        const bool fwd = kr.code < 4 || kr.code == 8 || kr.code == 10;
        key_meta[k0 + k] = uint8_t(kr.kind | (fwd ? 4 : 0) | (kr.overlong ? 8 : 0));
        key_group[k0 + k] = kr.group;
        key_final[k0 + k] = kr;
        key_col[k0 + k] = c;
        int sl;
        if (kr.kind == 1) sl = 2 + int(kr.len);
        else {
            const long long ri = (long long)col_pos[c] - ref_start;
            long long take = min((long long)kr.len + 1, (long long)max_indel);
            take = min(take, ref_len - ri);
            sl = 1 + int(take > 0 ? take : 0);
        }
        key_len[k0 + k] = sl;
    }
}

__global__ void k_keys_str(int n_keys, const KeyRec* __restrict__ key_final, const int* __restrict__ key_col, const long long* __restrict__ str_off,
                           const uint8_t* __restrict__ lin, const DevRead* __restrict__ reads, const int* __restrict__ rid,
                           const int32_t* __restrict__ col_pos, const char* __restrict__ ref, long long ref_start, char* __restrict__ out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_keys) return;
    const KeyRec kr = key_final[k];
    char* o = out + str_off[k];
    const int n = int(str_off[k + 1] - str_off[k]);
    static const char kAnchor[] = "ACGTACGT*#NN";
    static const char kNt16[] = "NACMGRSVTWYHKDBN";          // upper case, '=' -> N
    if (kr.kind == 1) {
        o[0] = 'I';
        o[1] = kAnchor[kr.code];
        const uint8_t* seq = lin + reads[rid[kr.read]].seq_off;
        for (int t = 0; t + 2 < n; ++t) { const int q = int(kr.q) + t; o[2 + t] = kNt16[(seq[q >> 1] >> ((~q & 1) << 2)) & 15]; }
    } else {
        o[0] = 'D';
        const long long ri = (long long)col_pos[key_col[k]] - ref_start;
        for (int t = 0; t + 1 < n; ++t) { char ch = ref[ri + t]; if (ch >= 'a' && ch <= 'z') ch = char(ch - 32); o[1 + t] = ch; }
    }
}

}  // namespace

struct cto_dev_pileup {
    RecordStream rs;                     // inflated blocks -> record offsets (bam_records.h); its upload block carries the intervals
                                         // and the reference window too, its event serves every wait of the driver
    DevBuf tile_b;                       // tile sums of the column scan (next to rs.tile_a, rs.tile_tot)
    DevBuf reads, rid, live, diff, slot_col, col_slot, col_off, col_pos, col_ref, cursor, tmp,
        entries, nkc, keyrec, key_off, key_meta, key_group, key_final, key_col, key_len, str_off, key_str;
    PinBuf h_stage;                      // page-locked landing area of the small arrays that go back to the host (a copy to pageable
                                         // memory blocks - and spins - until everything queued in front of it is done)
};

extern "C" int cto_dev_pileup_create(cto_dev_pileup** out) try {
    CTO_REQUIRE(out, CTO_EINVAL, "cto_dev_pileup_create: null argument");
    std::unique_ptr<cto_dev_pileup> c(new cto_dev_pileup());
    if (const int rc = c->rs.init()) return rc;
    *out = c.release();
    return CTO_OK;
}
CTO_CATCH("cto_dev_pileup_create", int)

extern "C" void cto_dev_pileup_destroy(cto_dev_pileup* c) { delete c; }

extern "C" int cto_pileup_device(cto_dev_pileup* cx, const void* d_inflated, const cto_bgzf_block* h_blocks, int64_t n_blocks,
                                 const uint64_t* rec_voffs, int64_t n_starts, int32_t tid, int64_t start, int64_t end, const int64_t* bed,
                                 int64_t n_bed, const char* ref_seq, int64_t ref_start, size_t ref_len, int excl_flags, int min_mq,
                                 int max_depth, int max_indel_length, void* stream, cto_pack_view* dev_view, cto_pack** host_lite,
                                 int* fallback) try {
    CTO_REQUIRE(cx && d_inflated && h_blocks && n_blocks > 0 && rec_voffs && n_starts > 0 && ref_seq && dev_view && host_lite && fallback,
                CTO_EINVAL, "cto_pileup_device: bad argument");
    CTO_REQUIRE(start >= 1 && end >= start && end < (int64_t(1) << 31), CTO_EINVAL, "cto_pileup_device: bad region");
    hipStream_t s = static_cast<hipStream_t>(stream);
    *fallback = 0;
    *host_lite = nullptr;
    // ---- host-side tables: block -> linear offset, record starts as linear offsets, requested intervals ----
    SpanTables tables;
    tables.lay_out(h_blocks, n_blocks);
    tables.map_starts(h_blocks, n_blocks, rec_voffs, n_starts);
    CTO_REQUIRE(tables.len < (int64_t(1) << 32) - 65536, CTO_EUNSUPPORTED, "cto_pileup_device: more than 4 GiB of alignment records in one chunk");
    CTO_REQUIRE(tables.n_chains > 0, CTO_EINVAL, "cto_pileup_device: no record start inside the inflated span");
    std::vector<int> ivs;                                        // lo[], hi[], base[] back to back
    {
        std::vector<std::pair<int64_t, int64_t>> v;
        if (bed) for (int64_t i = 0; i < n_bed; ++i) v.push_back({std::max<int64_t>(bed[2 * i], start - 1), std::min<int64_t>(bed[2 * i + 1], end)});
        else v.push_back({start - 1, end});
        std::vector<int> lo, hi, base;
        int64_t total = 0;
        for (auto& p : v)
            if (p.second > p.first) { lo.push_back(int(p.first)); hi.push_back(int(p.second)); base.push_back(int(total)); total += p.second - p.first; }
        CTO_REQUIRE(total < (int64_t(1) << 30), CTO_EUNSUPPORTED, "cto_pileup_device: too many requested positions");
        ivs = lo;
        ivs.insert(ivs.end(), hi.begin(), hi.end());
        ivs.insert(ivs.end(), base.begin(), base.end());
        ivs.push_back(int(total));
    }
    const int n_iv = int((ivs.size() - 1) / 3), total = ivs.back();
    RecordStream& rs = cx->rs;
    auto point_view = [&] {              // the pack's arrays where the context holds them
        dev_view->col_pos = cx->col_pos.as<int32_t>();
        dev_view->col_ref = cx->col_ref.as<uint8_t>();
        dev_view->col_off = cx->col_off.as<int64_t>();
        dev_view->key_off = cx->key_off.as<int32_t>();
        dev_view->entries = cx->entries.as<uint32_t>();
        dev_view->key_meta = cx->key_meta.as<uint8_t>();
        dev_view->key_group = cx->key_group.as<int32_t>();
    };
    auto empty_result = [&]() -> int {
        std::unique_ptr<cto_pack> p(new cto_pack());
        p->col_off.push_back(0);
        p->key_off.push_back(0);
        p->key_str_off.push_back(0);
        memset(dev_view, 0, sizeof(*dev_view));
        // an empty pack still has its two one-element offset arrays (col_off = key_off = {0}) and valid pointers everywhere
        int rc0;
        if ((rc0 = cx->col_off.ensure(64)) || (rc0 = cx->key_off.ensure(64)) || (rc0 = cx->col_pos.ensure(64)) || (rc0 = cx->col_ref.ensure(64)) ||
            (rc0 = cx->entries.ensure(64)) || (rc0 = cx->key_meta.ensure(64)) || (rc0 = cx->key_group.ensure(64)))
            return rc0;
        CTO_HIP(hipMemsetAsync(cx->col_off.p, 0, 64, s));
        CTO_HIP(hipMemsetAsync(cx->key_off.p, 0, 64, s));
        if ((rc0 = rs.wait(s))) return rc0;
        point_view();
        *host_lite = p.release();
        return CTO_OK;
    };
    if (total == 0) return empty_result();
    int rc;
    if ((rc = cx->diff.ensure(size_t(total + 1) * 4)) || (rc = cx->slot_col.ensure(size_t(total) * 4)) ||
        (rc = cx->col_slot.ensure(size_t(total) * 4)) || (rc = cx->col_off.ensure(size_t(total + 1) * 8)))
        return rc;
    CTO_HIP(hipMemsetAsync(cx->diff.p, 0, size_t(total + 1) * 4, s));
    // ---- the record stream and its boundaries; the intervals and the reference window ride in its upload block ----
    UploadParts extra;
    extra.add(ivs.data(), ivs.size() * 4);
    extra.add(ref_seq, ref_len);
    if ((rc = rs.begin(s, d_inflated, h_blocks, n_blocks, tables, extra))) return rc;
    const Flags* hf = rs.h_flags.as<Flags>();
    Flags* const fl = rs.fl;
    const int* d_ivs = rs.extra<int>(0);
    const char* d_ref = rs.extra<char>(1);
    const uint8_t* lin = rs.lin.as<uint8_t>();
    if (hf->bad_crc) {
        set_error("cto_pileup_device: the BGZF block at file offset %llu fails its CRC-32", (unsigned long long)h_blocks[hf->bad_crc - 1].file_off);
        return CTO_EINVAL;
    }
    if (hf->bad_chain) {
        set_error(hf->bad_chain == 2 ? "cto_pileup_device: bad alignment block size" : "cto_pileup_device: an index offset is not a record boundary");
        return CTO_EINVAL;
    }
    const int n_rec = hf->n_rec;
    if (n_rec == 0) return empty_result();
    if ((rc = cx->reads.ensure(size_t(n_rec) * sizeof(DevRead))) || (rc = cx->rid.ensure(size_t(n_rec) * 4)) ||
        (rc = cx->live.ensure(size_t(n_rec + 1) * 4)))
        return rc;
    CTO_HIP(hipMemsetAsync(cx->live.p, 0, size_t(n_rec + 1) * 4, s));
    if ((rc = rs.offsets(s, n_rec))) return rc;
    hipLaunchKernelGGL(k_parse, dim3(unsigned(cdiv(n_rec, 128))), dim3(128), 0, s, lin, rs.rec_off.as<uint32_t>(), n_rec, tid, int(start - 1), int(end),
                       excl_flags, min_mq, cx->reads.as<DevRead>(), fl);
    hipLaunchKernelGGL(k_compact, dim3(1), dim3(1024), 0, s, cx->reads.as<DevRead>(), n_rec, cx->rid.as<int>(), fl);
    hipLaunchKernelGGL(k_live_marks, dim3(unsigned(cdiv(n_rec, 128))), dim3(128), 0, s, cx->reads.as<DevRead>(), cx->rid.as<int>(), fl, cx->live.as<int>());
    hipLaunchKernelGGL(k_live_max, dim3(1), dim3(1024), 0, s, cx->live.as<int>(), fl);
    Ivs iv{d_ivs, d_ivs + n_iv, d_ivs + 2 * n_iv, n_iv, total};
    hipLaunchKernelGGL(k_cover, dim3(unsigned(cdiv(n_rec, 128))), dim3(128), 0, s, cx->reads.as<DevRead>(), cx->rid.as<int>(), fl, iv, cx->diff.as<int>());
    {
        const int tiles = int(cdiv(total, SCAN_TILE));
        if ((rc = rs.tile_a.ensure(size_t(tiles + 1) * 8)) || (rc = cx->tile_b.ensure(size_t(tiles + 1) * 16)) || (rc = rs.tile_tot.ensure(64))) return rc;
        long long* ta = rs.tile_a.as<long long>();
        long long* tb = cx->tile_b.as<long long>();
        long long* tt = rs.tile_tot.as<long long>();
        hipLaunchKernelGGL(k_tile_sums, dim3(unsigned(tiles)), dim3(1024), 0, s, cx->diff.as<int>(), total, ta);
        hipLaunchKernelGGL(k_scan_tiles, dim3(1), dim3(1024), 0, s, ta, tiles, 1, tt + 2);
        hipLaunchKernelGGL(k_columns_count, dim3(unsigned(tiles)), dim3(1024), 0, s, cx->diff.as<int>(), total, ta, tb);
        hipLaunchKernelGGL(k_scan_tiles, dim3(1), dim3(1024), 0, s, tb, tiles, 2, tt);
        hipLaunchKernelGGL(k_columns_write, dim3(unsigned(tiles)), dim3(1024), 0, s, cx->diff.as<int>(), total, ta, tb, tt, cx->slot_col.as<int>(),
                           cx->col_slot.as<int>(), cx->col_off.as<long long>(), fl);
    }
    CTO_HIP(hipGetLastError());
    if ((rc = rs.fetch_flags(s))) return rc;
    const int lim = hf->stop_idx;
    if (hf->err_idx < lim) { set_error("cto_pileup_device: alignment record shorter than its fields, or running past 2^31 - 1"); return CTO_EINVAL; }
    if (hf->paired_idx < lim || hf->skip_idx < lim || hf->deep_col || (max_depth > 0 && hf->max_live >= max_depth) || hf->max_live >= FILL_LIVE_MAX) {
        *fallback = 1;
        return CTO_OK;
    }
    const int n_cols = hf->n_cols;
    const long long n_entries = hf->n_entries;
    if (n_cols == 0) return empty_result();
    if ((rc = cx->col_pos.ensure(size_t(n_cols) * 4)) || (rc = cx->col_ref.ensure(size_t(n_cols))) || (rc = cx->cursor.ensure(size_t(n_cols) * 4)) ||
        (rc = cx->tmp.ensure(size_t(n_entries) * sizeof(TmpEnt))) || (rc = cx->entries.ensure(size_t(n_entries) * 4)) ||
        (rc = cx->nkc.ensure(size_t(n_cols + 1) * 4)) || (rc = cx->keyrec.ensure(size_t(n_entries) * sizeof(KeyRec))) || (rc = cx->key_off.ensure(size_t(n_cols + 1) * 4)))
        return rc;
    CTO_HIP(hipMemsetAsync(cx->cursor.p, 0, size_t(n_cols) * 4, s));
    hipLaunchKernelGGL(k_col_meta, dim3(unsigned(cdiv(n_cols, 256))), dim3(256), 0, s, cx->col_slot.as<int>(), n_cols, iv, d_ref, (long long)ref_start,
                       (long long)ref_len, cx->col_pos.as<int32_t>(), cx->col_ref.as<uint8_t>(), fl);
    int live_cap = 64;
    while (live_cap <= hf->max_live) live_cap <<= 1;
    hipLaunchKernelGGL(k_fill, dim3(unsigned(((hf->n_valid + 7) >> 3) << 3)), dim3(256), size_t(live_cap) * 8 * sizeof(int), s, live_cap, lin, cx->reads.as<DevRead>(), cx->rid.as<int>(), fl, iv,
                       cx->slot_col.as<int>(), cx->col_off.as<long long>(), cx->cursor.as<int>(), cx->entries.as<uint32_t>(), cx->tmp.as<TmpEnt>(), d_ref,
                       (long long)ref_start, (long long)ref_len);
    hipLaunchKernelGGL(k_order, dim3(unsigned(std::min<long long>(cdiv(n_cols, 64), 65536))), dim3(64), 0, s, lin, cx->reads.as<DevRead>(), cx->rid.as<int>(),
                       n_cols, cx->col_off.as<long long>(), cx->cursor.as<int>(), cx->tmp.as<TmpEnt>(), cx->entries.as<uint32_t>(), cx->nkc.as<int>(),
                       cx->keyrec.as<KeyRec>(), max_indel_length, fl);
    if ((rc = rs.scan(s, cx->nkc.as<int>(), n_cols, cx->key_off.as<int>(), &fl->n_keys))) return rc;
    CTO_HIP(hipGetLastError());
    if ((rc = rs.fetch_flags(s))) return rc;
    if (hf->ref_oob) { set_error("cto_pileup_device: a covered position lies outside the supplied reference"); return CTO_EINVAL; }
    if (hf->many_keys || hf->deep_col) { *fallback = 1; return CTO_OK; }          // deep_col here: more than FILL_LIVE reads open at a read's start
    const int n_keys = hf->n_keys;
    std::unique_ptr<cto_pack> lite(new cto_pack());
    lite->col_pos.resize(size_t(n_cols));
    lite->col_ref.resize(size_t(n_cols));
    lite->key_off.resize(size_t(n_cols) + 1);
    lite->col_off.assign(1, 0);
    lite->key_str_off.assign(size_t(n_keys) + 1, 0);
    if ((rc = cx->key_meta.ensure(16)) || (rc = cx->key_group.ensure(16))) return rc;      // valid pointers for a pack without keys
    if (n_keys > 0) {
        if ((rc = cx->key_meta.ensure(size_t(n_keys))) || (rc = cx->key_group.ensure(size_t(n_keys) * 4)) || (rc = cx->key_final.ensure(size_t(n_keys) * sizeof(KeyRec))) ||
            (rc = cx->key_col.ensure(size_t(n_keys) * 4)) || (rc = cx->key_len.ensure(size_t(n_keys + 1) * 4)) || (rc = cx->str_off.ensure(size_t(n_keys + 1) * 8)))
            return rc;
        hipLaunchKernelGGL(k_keys_meta, dim3(unsigned(cdiv(n_cols, 256))), dim3(256), 0, s, n_cols, cx->col_off.as<long long>(), cx->key_off.as<int>(),
                           cx->keyrec.as<KeyRec>(), cx->col_pos.as<int32_t>(), (long long)ref_start, (long long)ref_len, max_indel_length,
                           cx->key_meta.as<uint8_t>(), cx->key_group.as<int32_t>(), cx->key_final.as<KeyRec>(), cx->key_col.as<int>(), cx->key_len.as<int>());
        if ((rc = rs.scan(s, cx->key_len.as<int>(), n_keys, cx->str_off.as<long long>(), &fl->key_str_bytes))) return rc;
        CTO_HIP(hipGetLastError());
        if ((rc = rs.fetch_flags(s))) return rc;
        const long long sb = hf->key_str_bytes;
        if ((rc = cx->key_str.ensure(size_t(sb) + 16))) return rc;
        hipLaunchKernelGGL(k_keys_str, dim3(unsigned(cdiv(n_keys, 128))), dim3(128), 0, s, n_keys, cx->key_final.as<KeyRec>(), cx->key_col.as<int>(),
                           cx->str_off.as<long long>(), lin, cx->reads.as<DevRead>(), cx->rid.as<int>(), cx->col_pos.as<int32_t>(), d_ref,
                           (long long)ref_start, cx->key_str.as<char>());
        CTO_HIP(hipGetLastError());
        lite->key_str.resize(size_t(sb));
        lite->key_meta.resize(size_t(n_keys));
        lite->key_group.resize(size_t(n_keys));
        static_assert(sizeof(long long) == sizeof(int64_t), "");
    }
    {
        // everything the host keeps of the pack, through ONE page-locked landing area and one sleeping wait
        const size_t sb = lite->key_str.size(), nk = size_t(n_keys), nc = size_t(n_cols);
        const size_t bytes[7] = {nk ? (nk + 1) * 8 : 0, sb, nk, nk * 4, nc * 4, nc, (nc + 1) * 4};
        const void* src[7] = {cx->str_off.p, cx->key_str.p, cx->key_meta.p, cx->key_group.p, cx->col_pos.p, cx->col_ref.p, cx->key_off.p};
        void* dst[7] = {lite->key_str_off.data(), sb ? &lite->key_str[0] : nullptr, lite->key_meta.data(), lite->key_group.data(), lite->col_pos.data(),
                        lite->col_ref.data(), lite->key_off.data()};
        size_t off[7], total = 0;
        for (int i = 0; i < 7; ++i) { off[i] = total; total += (bytes[i] + 63) / 64 * 64; }
        if ((rc = cx->h_stage.ensure(total + 64))) return rc;
        char* hs = cx->h_stage.as<char>();
        for (int i = 0; i < 7; ++i)
            if (bytes[i]) CTO_HIP(hipMemcpyAsync(hs + off[i], src[i], bytes[i], hipMemcpyDeviceToHost, s));
        if ((rc = rs.wait(s))) return rc;
        for (int i = 0; i < 7; ++i)
            if (bytes[i]) memcpy(dst[i], hs + off[i], bytes[i]);
    }
    dev_view->n_cols = n_cols;
    dev_view->n_entries = n_entries;
    dev_view->n_keys = n_keys;
    point_view();
    *host_lite = lite.release();
    return CTO_OK;
}
CTO_CATCH("cto_pileup_device", int)

// test / tool aid: n bytes of device memory to the host (synchronous)
extern "C" int cto_device_read(const void* d_src, void* h_dst, size_t n) {
    CTO_REQUIRE((d_src && h_dst) || n == 0, CTO_EINVAL, "cto_device_read: null argument");
    if (n) CTO_HIP(hipMemcpy(h_dst, d_src, n, hipMemcpyDeviceToHost));
    return CTO_OK;
}
