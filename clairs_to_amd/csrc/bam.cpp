// BAM -> column pack producer: what `samtools mpileup --reverse-del --output-MQ -r ctg:s-e --min-MQ 0
// --min-BQ 0 -l <bed> --excl-flags 2316 [--max-depth N]` followed by the text tokeniser would yield, without the text.
//
// PARITY UNPINNED: neither samtools nor htslib exists on the build or GPU boxes, so this reader is validated only against
// an independent restatement of the pileup rules below on BAM files written by the test-suite itself
// (tests/bamutil.py, tests/test_bam_reader.py).  The drivers keep `samtools mpileup` as their default producer.
//
// Pileup rules implemented (SAM/BAM specification v1 sections 4.2, 5.1-5.3 for the formats; samtools-mpileup(1) and
// SURVEY.md Appendix B for the column semantics):
//   * a record is used if it is mapped to the region's reference, (flag & excl_flags) == 0, MAPQ >= min_mq, has a CIGAR
//     and SEQ, and - as mpileup does without -A - is not an "orphan" (PAIRED set without PROPER_PAIR);
//   * reads enter a column in file order (= coordinate order, ties by file position);
//   * M / = / X : one read-base per reference position, base letter upper case on the forward strand, lower case on the
//     reverse strand ('=' resolves to the reference base), BQ = QUAL at that query position;
//   * D : placeholder '*' (forward) / '#' (reverse, --reverse-del) at every deleted position, carrying the BQ of the
//     query base that follows the deletion (0 past the end of the read);
//   * the last aligned base before an I (or D) carries the indel: inserted bases in the strand's case, or len x 'N'/'n'
//     for a deletion (no -f: deleted bases print as N); an insertion that is not preceded by an aligned base of the
//     same read (start of read, after a clip / skip / deletion) is not reported;
//   * N (reference skip) contributes nothing (samtools prints '>' / '<', which the reference's decoder ignores);
//   * S / H / P consume as the specification says and contribute nothing;
//   * MQ and BQ are capped at 93, the largest value mpileup's phred+33 characters can carry;
//   * a read is dropped when `max_depth` reads are already active at its start (htslib's per-file maxcnt); the outcome does
//     not depend on the number of decoding threads (a call whose ranges hit the cap is redone unsplit);
//   * rows exist only for positions covered by >= 1 read-base or placeholder, inside [start, end] and inside the BED
//     intervals when given.
//   * read-pair overlaps (mpileup without -x, as the reference runs it): where both mates of a pair have an aligned base at a
//     position, the first mate's base keeps min(200, qa + qb) when they agree and the better base keeps 0.8 x its quality
//     when they differ; the other base's quality becomes 0 (soften_overlap below).  Paired-end short reads only.  WHICH mate
//     keeps the base when they agree is a second unpinned point (advisor, round 2): recent htslib releases may pick it per read
//     name instead of always favouring the first - with no htslib on either box this cannot be settled here, so for paired-end
//     input `samtools` stays the reference producer and `--bam_reader native|gpu` is offered for the long-read platforms.
// Not implemented (documented deviations): BAQ (needs -f, which the reference does not pass), CRAM, multi-file input.
//
// I/O: the file is mapped; every BGZF block is inflated (libdeflate when the runtime library is present, else zlib) and checked
// against the CRC-32 of its gzip trailer, as htslib does.  Blocks a caller inflated elsewhere (cto_pack_from_bam_inflated: on the
// device, csrc/inflate.hip) are looked up by file offset and CRC-checked the same way.  Columns are built in runs of requested
// positions, read by read (Producer below).
// The formats themselves - BGZF, the index, the grammar of an alignment record - are read by csrc/bam_host.h; what is here are its consumers.
#include <atomic>
#include <chrono>
#include <deque>
#include <map>
#include <memory>
#include <thread>
#include <unordered_map>

#include "bam_host.h"
#include "deflate_host.h"
#include "deflate_internal.h"
#include "hap_internal.h"
#include "pack_internal.h"

using namespace cto;

namespace {

// ------------------------------------------------------------------------------------------------ records + pileup
struct Read {
    int32_t pos = 0;            // 0-based leftmost
    int32_t end = 0;            // 0-based exclusive reference end
    uint8_t mapq = 0;
    bool rev = false;
    std::vector<uint32_t> cigar;
    std::vector<uint8_t> raw;   // the alignment record as read; packed SEQ (4 bits per base) and QUAL are decoded on demand, since a
                                // BED-restricted pileup touches a small part of a long read
    int32_t l_seq = 0;
    bool no_qual = false;
    std::string mate_key;       // QNAME of a paired read (empty otherwise): mates find each other through it
    size_t seq_off = 0, qual_off = 0;   // where SEQ and QUAL start in `raw` (the whole record is kept: no second copy)
    int base4(int q) const { return (raw[seq_off + size_t(q >> 1)] >> ((~q & 1) << 2)) & 15; }
    int bq(int q) const { return (no_qual || q >= l_seq) ? 0 : std::min(int(raw[qual_off + size_t(q)]), 93); }
    uint8_t* qual_at(int q) { return &raw[qual_off + size_t(q)]; }
    // query index of the aligned base (M / = / X) at 0-based reference position rpos, or -1 (deletion, skip, outside the read)
    int query_at(int32_t rpos) const {
        int32_t rp = pos, qp = 0;
        for (uint32_t c : cigar) {
            const int len = int(c >> 4), opc = int(c & 15);
            const bool cons_ref = consumes_ref(opc);
            const bool cons_q = consumes_query(opc);
            if (cons_ref && rpos < rp + len) return (cons_q && rpos >= rp) ? qp + (rpos - rp) : -1;
            if (cons_ref) rp += len;
            if (cons_q) qp += len;
        }
        return -1;
    }
    // cursor: CIGAR op index, offset inside it, reference / query positions at the start of the op
    size_t op = 0;
    int32_t op_ref = 0, op_q = 0;
    // reference positions op_ref <= rpos < fast_end lie inside the current op, which is an aligned run (M / = / X), and are not
    // its last base (after which an indel may follow): the column loop packs them without looking at the CIGAR
    int32_t fast_end = INT32_MIN;
};

// entry code of a 4-bit BAM base on the forward strand: A C G T -> 0..3, '=' -> -1 (take the reference base), IUPAC codes -> N
const int8_t kNibCode[16] = {-1, 0, 1, 10, 2, 10, 10, 10, 3, 10, 10, 10, 10, 10, 10, 10};

const char kNt16[] = "=ACMGRSVTWYHKDBN";

// Read-pair overlap handling of `samtools mpileup` (on unless -x / --ignore-overlaps-removal; the reference never passes -x,
// SURVEY.md App. B): where the two mates of a pair cover the same reference position with an aligned base each, one base is
// kept and the other nullified by a base quality of 0 (samtools-mpileup(1), "--ignore-overlaps-removal"); the kept base gets
// the sum of both qualities (capped at 200) when the mates agree, 0.8 x the larger quality when they differ (htslib's
// tweak_overlap_quality).  `a` is the mate that entered the pileup first.  A quality-0 base still prints under --min-BQ 0 - it
// is the AFF pass's --min_bq and the LBQ channels that see the difference.  Long reads are unpaired: nothing happens.
void soften_overlap(Read& a, Read& b) {
    if (a.no_qual || b.no_qual) return;
    const int32_t lo = std::max(a.pos, b.pos), hi = std::min(a.end, b.end);
    for (int32_t rp = lo; rp < hi; ++rp) {
        const int qa = a.query_at(rp), qb = b.query_at(rp);
        if (qa < 0 || qb < 0) continue;
        uint8_t* pa = a.qual_at(qa);
        uint8_t* pb = b.qual_at(qb);
        if (a.base4(qa) == b.base4(qb)) {
            const int s = int(*pa) + int(*pb);
            *pa = uint8_t(s > 200 ? 200 : s);
            *pb = 0;
        } else if (*pa >= *pb) {
            *pa = uint8_t(0.8 * *pa);
            *pb = 0;
        } else {
            *pb = uint8_t(0.8 * *pb);
            *pa = 0;
        }
    }
}

struct Producer {
    cto_pack* p;
    ColumnScratch sc;
    const char* ref_seq;
    int64_t ref_start;
    size_t ref_len;
    int max_indel;
    // Columns are built in runs of up to RUN consecutive requested positions, read by read: a read's bases inside an aligned
    // CIGAR run go to their columns in one tight loop (sequence, qualities and cursor stay in cache), and the order of the
    // entries inside a column is still the order of the reads in `active` (= the order mpileup prints them in).
    static constexpr int RUN = 64;
    std::vector<uint32_t> ents[RUN];    // per column of the current run: packed entries, indel fields still empty
    std::vector<IndelAt> indels[RUN];   // ... and which of them carry an indel
    std::deque<std::string> arena;      // inserted sequences of the current run (IndelAt::seq points into these)
    std::string nbuf_up, nbuf_lo;       // runs of 'N' / 'n' for deletion keys
    std::string err;

    void begin_run(int ncol) {
        for (int c = 0; c < ncol; ++c) { ents[c].clear(); indels[c].clear(); }
        if (!arena.empty()) arena.clear();
    }
    // deletion keys are runs of 'N' / 'n' out of two shared buffers that emit_one() grows on demand
    void seal_column(int c) {
        for (IndelAt& it : indels[c])
            if (it.kind == 2) {
                const uint32_t code = ents[c][size_t(it.idx)] & 15u;
                const bool rev = (code >= 4 && code <= 7) || code == 9 || code == 11;
                it.seq = (rev ? nbuf_lo : nbuf_up).data();
            }
    }
    // the read's contribution to the columns of reference positions lo .. hi (0-based, inside the read); run0 = position of column 0
    void emit_run(Read& r, int32_t lo, int32_t hi, int32_t run0) {
        const int mq = std::min(int(r.mapq), 93);              // mpileup prints min(MAPQ, 93) + 33, likewise for BQ
        int32_t rp = lo;
        while (rp <= hi) {
            if (rp < r.fast_end) {                             // inside an aligned run, not its last base: no CIGAR work
                const int32_t stop = std::min(hi + 1, r.fast_end);
                int q = r.op_q + (rp - r.op_ref);
                for (; rp < stop; ++rp, ++q) ents[rp - run0].push_back(pack_entry(code_at(r, q, rp), r.bq(q), mq));
            } else {
                emit_one(r, rp, rp - run0, mq);
                ++rp;
            }
        }
    }
    int code_at(const Read& r, int q, int32_t rpos) const {
        int code = kNibCode[r.base4(q)];
        if (code < 0) {                                        // '=': the reference base (mpileup prints IUPAC codes; the decoder
            const int64_t ri = int64_t(rpos) + 1 - ref_start;   // ignores all but ACGTN)
            const char b = (ri >= 0 && size_t(ri) < ref_len) ? up(ref_seq[ri]) : 'N';
            code = b == 'A' ? 0 : (b == 'C' ? 1 : (b == 'G' ? 2 : (b == 'T' ? 3 : 10)));
        }
        return r.rev ? code + ((code < 4) ? 4 : 1) : code;     // A..T -> a..t, N -> n
    }
    // advances the read's cursor to reference position `rpos` (0-based) and appends its contribution to column `col`
    void emit_one(Read& r, int32_t rpos, int col, int mq) {
        std::vector<uint32_t>& ents = this->ents[col];
        std::vector<IndelAt>& indels = this->indels[col];
        while (r.op < r.cigar.size()) {
            const uint32_t c = r.cigar[r.op];
            const int len = int(c >> 4), opc = int(c & 15);
            const bool cons_ref = consumes_ref(opc);
            const bool cons_q = consumes_query(opc);
            if (cons_ref && rpos < r.op_ref + len) break;
            if (cons_ref) r.op_ref += len;
            if (cons_q) r.op_q += len;
            ++r.op;
        }
        r.fast_end = INT32_MIN;
        if (r.op >= r.cigar.size()) return;
        const uint32_t c = r.cigar[r.op];
        const int len = int(c >> 4), opc = int(c & 15);
        const int off = rpos - r.op_ref;
        if (opc == 3) return;                                  // N: reference skip, nothing in the pack
        if (opc == 2) {                                        // D: placeholder
            ents.push_back(pack_entry(r.rev ? 9 : 8, r.bq(r.op_q), mq));
            return;
        }
        // aligned base
        r.fast_end = r.op_ref + len - 1;
        const int q = r.op_q + off;
        ents.push_back(pack_entry(code_at(r, q, rpos), r.bq(q), mq));
        if (off == len - 1) {                                  // last base of the op: does an indel follow?
            size_t nx = r.op + 1;
            while (nx < r.cigar.size() && (r.cigar[nx] & 15) == 6) ++nx;    // P
            if (nx < r.cigar.size()) {
                const int nop = int(r.cigar[nx] & 15), nlen = int(r.cigar[nx] >> 4);
                if (nop == 1) {
                    arena.emplace_back();
                    std::string& s = arena.back();
                    for (int i = 0; i < nlen; ++i) {
                        char ib = kNt16[r.base4(q + 1 + i)];
                        if (ib == '=') ib = 'N';
                        s.push_back(r.rev ? char(ib | 0x20) : ib);
                    }
                    indels.push_back(IndelAt{int(ents.size()) - 1, 1, s.data(), nlen});
                } else if (nop == 2) {
                    std::string& nb = r.rev ? nbuf_lo : nbuf_up;      // may grow again within this column: the pointer is set
                    if (int(nb.size()) < nlen) nb.assign(size_t(nlen), r.rev ? 'n' : 'N');      // by seal_column()
                    indels.push_back(IndelAt{int(ents.size()) - 1, 2, nullptr, nlen});
                }
            }
        }
    }
};

double now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

bool in_bed(const int64_t* bed, int64_t n_bed, int64_t pos1, int64_t* cursor) {
    if (!bed) return true;
    const int64_t p0 = pos1 - 1;
    while (*cursor < n_bed && bed[2 * *cursor + 1] <= p0) ++*cursor;     // intervals sorted by start, merged by the caller
    return *cursor < n_bed && bed[2 * *cursor] <= p0;
}

// One position range [start, end] on one thread: own file handle, own index query.  Errors go through set_error (thread-local).
int pack_from_bam_range(const char* bam_path, const char* bai_path, const char* ctg_name, int64_t start, int64_t end,
                        const int64_t* bed, int64_t n_bed, const char* ref_seq, int64_t ref_start, size_t ref_len,
                        int excl_flags, int min_mq, int max_depth, int max_indel_length, const PreInflated& pre, cto_pack** out,
                        bool* cap_hit = nullptr) {
    BamRegion rg;                        // 0-based half-open region
    CTO_REQUIRE(rg.open("cto_pack_from_bam", bam_path, bai_path, ctg_name, start - 1, end, false, false, pre), CTO_EINVAL, "%s", rg.err.c_str());
    std::unique_ptr<cto_pack> pk(new cto_pack());
    pack_begin(pk.get(), 1 << 16, 1 << 10);
    Producer pr;
    pr.p = pk.get();
    pr.ref_seq = ref_seq;
    pr.ref_start = ref_start;
    pr.ref_len = ref_len;
    pr.max_indel = max_indel_length;

    std::deque<Read> active;
    int64_t prev_start = 0;              // 0-based start of the last record that reached this point (see the flush below)
    int64_t next_col = start;            // next 1-based position to emit
    int64_t bed_cursor = 0;
    auto flush_until = [&](int64_t limit1) -> int {   // emit columns next_col .. limit1 (1-based, inclusive)
        while (next_col <= limit1) {
            while (!active.empty() && active.front().end <= next_col - 1) active.pop_front();
            if (active.empty()) { next_col = limit1 + 1; break; }       // nothing can cover the positions up to the limit
            int64_t last = std::min<int64_t>(limit1, next_col + Producer::RUN - 1);     // run of requested positions next_col .. last
            if (bed) {
                if (!in_bed(bed, n_bed, next_col, &bed_cursor)) {
                    next_col = bed_cursor < n_bed ? std::max<int64_t>(next_col + 1, bed[2 * bed_cursor] + 1) : limit1 + 1;
                    continue;
                }
                last = std::min<int64_t>(last, bed[2 * bed_cursor + 1]);      // 1-based inclusive end of the interval
            }
            const int ncol = int(last - next_col + 1);
            pr.begin_run(ncol);
            const int32_t lo0 = int32_t(next_col - 1), hi0 = int32_t(last - 1);
            size_t dead = 0;
            for (Read& r : active) {
                const int32_t lo = std::max(lo0, r.pos), hi = std::min(hi0, r.end - 1);
                if (lo <= hi) pr.emit_run(r, lo, hi, lo0);
                else dead += r.end <= lo0;
            }
            if (dead > 32 && dead * 2 > active.size())       // finished reads parked behind a long one: compact, keeping file order
                active.erase(std::remove_if(active.begin(), active.end(), [&](const Read& r) { return r.end <= lo0; }), active.end());
            for (int c = 0; c < ncol; ++c) {
                if (pr.ents[c].empty()) continue;
                pr.seal_column(c);
                const int64_t pos1 = next_col + c, ri = pos1 - ref_start;
                if (ri < 0 || size_t(ri) >= ref_len) {
                    set_error("cto_pack_from_bam: position %lld outside the supplied reference", (long long)pos1);
                    return CTO_EINVAL;
                }
                const int rc = append_column_packed(pr.p, pr.sc, pos1, ri, ref_seq, ref_len, max_indel_length, pr.ents[c].data(),
                                                    int(pr.ents[c].size()), pr.indels[c].data(), int(pr.indels[c].size()), &pr.err);
                if (rc != CTO_OK) { set_error("%s", pr.err.c_str()); return rc; }
            }
            next_col = last + 1;
        }
        return CTO_OK;
    };
    // Reads are NOT removed from `active` in end order (a deque in file order, popped only from the front): a long read
    // at the front keeps shorter finished ones behind it alive, which only costs the bounds check in the loop above.
    const bool timing = getenv("CTO_PACK_TIMING") != nullptr;
    double t_flush = 0.0, t_read = 0.0;
    const double t_begin = now();
    for (BamRecord b;;) {
        const double tr0 = timing ? now() : 0.0;
        const int got = rg.next(&b);
        if (timing) t_read += now() - tr0;
        CTO_REQUIRE(got >= 0, CTO_EINVAL, "%s", rg.err.c_str());
        if (got == 0) break;
        const int pos = b.pos, flag = b.flag;
        if ((flag & excl_flags) || (flag & 4) || b.mapq < min_mq || b.n_cig == 0 || b.l_seq <= 0 || pos < 0) continue;
        if ((flag & 1) && !(flag & 2)) continue;           // orphan (mpileup without -A)
        CTO_REQUIRE(rg.lay_out(&b), CTO_EINVAL, "%s", rg.err.c_str());
        const int enters = rg.enters(b);                   // no: inconsistent, reference-less or in front of the region
        CTO_REQUIRE(enters >= 0, CTO_EINVAL, "%s", rg.err.c_str());
        if (!enters) continue;
        Read r;
        r.pos = pos;
        r.end = int32_t(pos + b.rlen);
        r.mapq = uint8_t(b.mapq);
        r.rev = (flag & 16) != 0;
        r.cigar.resize(size_t(b.n_ops));
        for (int i = 0; i < b.n_ops; ++i) r.cigar[size_t(i)] = b.op(i);
        r.op_ref = pos;
        r.l_seq = b.l_seq;
        r.no_qual = b.ql[0] == 0xff;                                                           // QUAL absent
        r.seq_off = size_t(b.sq - rg.rec.data());
        r.qual_off = size_t(b.ql - rg.rec.data());
        r.raw.swap(rg.rec);                                // the record's buffer moves into the read (b's pointers stay valid: same
                                                           // heap block); the next record gets a fresh one
        // Columns strictly before the PREVIOUS accepted read's start are emitted now; those between the two starts wait for
        // the next record.  That is htslib's order (bam_plp_next hands out column p only once a read starting beyond p has
        // been pushed, so a read is pushed - and its mate's qualities are edited - while the iterator stands at the
        // previous read's start), and it shows in one place: a deletion placeholder of the first mate that lies between
        // the two starts already prints the edited quality of the base after the deletion.
        const double tf0 = timing ? now() : 0.0;
        const int rcf = flush_until(std::min<int64_t>(prev_start, end));     // 1-based columns <= prev_start (0-based) are final
        if (rcf != CTO_OK) return rcf;
        if (timing) t_flush += now() - tf0;
        if (max_depth > 0) {
            int live = 0;
            for (const Read& a : active) live += a.end > pos;
            if (live >= max_depth) { if (cap_hit) *cap_hit = true; continue; }
        }
        if ((flag & 1) && b.l_name > 1) {                  // paired: the mate may already be in the pileup
            r.mate_key.assign(reinterpret_cast<const char*>(b.name), size_t(b.l_name - 1));
            for (Read& a : active)
                if (a.end > pos && a.mate_key == r.mate_key) { soften_overlap(a, r); break; }
        }
        prev_start = pos;
        active.push_back(std::move(r));
    }
    const double tf1 = timing ? now() : 0.0;
    const int rcf = flush_until(end);
    if (rcf != CTO_OK) return rcf;
    if (timing)
        fprintf(stderr, "cto_pack_from_bam: total %.1f ms: read+inflate %.1f, pileup %.1f (libdeflate %d)\n", now() - t_begin, t_read,
                t_flush + now() - tf1, int(libdeflate().ok()));
    *out = pk.release();
    return CTO_OK;
}

// No C++ exception may cross the C ABI or leave a worker thread (std::terminate would take the host process down with it):
// allocation failures on hostile input (a record claiming 256 MB, a 4 GB index) come back as CTO_ENOMEM.
int pack_from_bam_impl(const char* bam_path, const char* bai_path, const char* ctg_name, int64_t start, int64_t end,
                       const int64_t* bed, int64_t n_bed, const char* ref_seq, int64_t ref_start, size_t ref_len,
                       int excl_flags, int min_mq, int max_depth, int max_indel_length, const PreInflated& pre, cto_pack** out) {
    CTO_REQUIRE(bam_path && ctg_name && ref_seq && out, CTO_EINVAL, "cto_pack_from_bam: null argument");
    CTO_REQUIRE(start >= 1 && end >= start, CTO_EINVAL, "cto_pack_from_bam: bad region %lld-%lld", (long long)start, (long long)end);
    CTO_REQUIRE(n_bed == 0 || bed, CTO_EINVAL, "cto_pack_from_bam: bed intervals missing");
    for (int64_t i = 1; i < n_bed; ++i)
        CTO_REQUIRE(bed[2 * i] >= bed[2 * i - 1], CTO_EINVAL, "cto_pack_from_bam: bed intervals must be sorted and non-overlapping");
    // Position ranges are independent (every range re-queries the index for the reads that overlap it), so a chunk is cut into
    // ranges of equal numbers of requested positions and piled up on several host threads, like the text tokeniser.  The
    // --max-depth cap is order dependent (a read is dropped when max_depth reads are live at its start), and a range does not see
    // the reads that ended before it: as long as NO range drops a read, no read is dropped in the unsplit order either (at a read's
    // start every live read reaches into the range that holds that start, so its count there is exact); as soon as one does, the
    // call is redone unsplit, so the pack never depends on how many threads the host happens to have.
    int64_t want = 0;                                       // requested positions inside [start, end]
    if (bed) {
        for (int64_t i = 0; i < n_bed; ++i) {
            const int64_t lo = std::max<int64_t>(bed[2 * i] + 1, start), hi = std::min<int64_t>(bed[2 * i + 1], end);
            if (hi >= lo) want += hi - lo + 1;
        }
    } else want = end - start + 1;
    unsigned nt = std::thread::hardware_concurrency();
    nt = std::max(1u, std::min(nt, 32u));
    nt = cto::pack_threads_or(nt);
    nt = unsigned(std::max<int64_t>(1, std::min<int64_t>(nt, want / 2000)));      // at least ~2000 positions per thread
    if (nt == 1)
        return pack_from_bam_range(bam_path, bai_path, ctg_name, start, end, bed, n_bed, ref_seq, ref_start, ref_len, excl_flags, min_mq,
                                   max_depth, max_indel_length, pre, out);
    // cut points: the position at which each thread's share of the requested positions begins
    std::vector<int64_t> cut(nt + 1, end + 1);
    cut[0] = start;
    {
        int64_t seen = 0;
        unsigned t = 1;
        auto feed = [&](int64_t lo, int64_t hi) {           // inclusive run of requested positions
            while (t < nt && seen + (hi - lo + 1) > want * t / nt) {
                cut[t] = lo + (want * t / nt - seen);
                ++t;
            }
            seen += hi - lo + 1;
        };
        if (bed) {
            for (int64_t i = 0; i < n_bed; ++i) {
                const int64_t lo = std::max<int64_t>(bed[2 * i] + 1, start), hi = std::min<int64_t>(bed[2 * i + 1], end);
                if (hi >= lo) feed(lo, hi);
            }
        } else feed(start, end);
    }
    std::vector<std::unique_ptr<cto_pack>> parts(nt);
    std::vector<int> rcs(nt, CTO_OK);
    std::vector<std::string> errs(nt);
    std::vector<char> capped(nt, 0);
    auto work = [&](unsigned t) {
        cto_pack* p = nullptr;
        if (cut[t + 1] - 1 < cut[t]) { parts[t].reset(new cto_pack()); pack_begin(parts[t].get(), 16, 16); return; }
        rcs[t] = guarded("cto_pack_from_bam", [&] {
            bool hit = false;
            const int rc = pack_from_bam_range(bam_path, bai_path, ctg_name, cut[t], cut[t + 1] - 1, bed, n_bed, ref_seq, ref_start, ref_len,
                                               excl_flags, min_mq, max_depth, max_indel_length, pre, &p, &hit);
            capped[t] = hit;
            return rc;
        });
        if (rcs[t] != CTO_OK) errs[t] = cto_last_error();
        parts[t].reset(p);
    };
    {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nt; ++t) th.emplace_back(work, t);
        for (auto& x : th) x.join();
    }
    for (unsigned t = 0; t < nt; ++t)
        if (capped[t]) {                                    // the cap bit somewhere: the unsplit order decides which reads go
            parts.clear();
            return pack_from_bam_range(bam_path, bai_path, ctg_name, start, end, bed, n_bed, ref_seq, ref_start, ref_len, excl_flags, min_mq,
                                       max_depth, max_indel_length, pre, out);
        }
    for (unsigned t = 0; t < nt; ++t)
        if (rcs[t] != CTO_OK) { set_error("%s", errs[t].c_str()); return rcs[t]; }
    std::string merr;
    std::unique_ptr<cto_pack> p = merge_parts(parts, &merr);
    CTO_REQUIRE(p != nullptr, CTO_EINVAL, "cto_pack_from_bam: %s", merr.c_str());
    *out = p.release();
    return CTO_OK;
}

}  // namespace

extern "C" int cto_pack_from_bam(const char* bam_path, const char* bai_path, const char* ctg_name, int64_t start, int64_t end,
                                  const int64_t* bed, int64_t n_bed, const char* ref_seq, int64_t ref_start, size_t ref_len,
                                  int excl_flags, int min_mq, int max_depth, int max_indel_length, cto_pack** out) {
    return guarded("cto_pack_from_bam", [&] {
        return pack_from_bam_impl(bam_path, bai_path, ctg_name, start, end, bed, n_bed, ref_seq, ref_start, ref_len, excl_flags, min_mq,
                                  max_depth, max_indel_length, PreInflated{}, out);
    });
}

extern "C" int cto_pack_from_bam_inflated(const char* bam_path, const char* bai_path, const char* ctg_name, int64_t start, int64_t end,
                                           const int64_t* bed, int64_t n_bed, const char* ref_seq, int64_t ref_start, size_t ref_len,
                                           int excl_flags, int min_mq, int max_depth, int max_indel_length, const uint8_t* inflated,
                                           size_t inflated_len, const cto_bgzf_block* blocks, int64_t n_blocks, cto_pack** out) {
    return guarded("cto_pack_from_bam_inflated", [&] {
        CTO_REQUIRE(n_blocks >= 0 && (n_blocks == 0 || (inflated && blocks)), CTO_EINVAL, "cto_pack_from_bam_inflated: null argument");
        for (int64_t i = 0; i < n_blocks; ++i) {
            CTO_REQUIRE(i == 0 || blocks[i].file_off > blocks[i - 1].file_off, CTO_EINVAL, "cto_pack_from_bam_inflated: block table not sorted");
            CTO_REQUIRE(blocks[i].isize <= 65536 && blocks[i].out_off <= inflated_len && blocks[i].isize <= inflated_len - blocks[i].out_off,
                        CTO_EINVAL, "cto_pack_from_bam_inflated: block %lld lies outside the inflated buffer", (long long)i);
        }
        PreInflated pre;
        pre.data = inflated;
        pre.blocks = blocks;
        pre.n = n_blocks;
        return pack_from_bam_impl(bam_path, bai_path, ctg_name, start, end, bed, n_bed, ref_seq, ref_start, ref_len, excl_flags, min_mq,
                                  max_depth, max_indel_length, pre, out);
    });
}

// ------------------------------------------------------------------------------------------------ allele counter, host path
// The plain definition of the allele-count rules (listed in full at the top of csrc/allelecount.hip, which holds the C entry point and
// the device path that is held equal to this one).  One call = one run of loci on one thread: every read that overlaps
// ctg:loci[0]-loci[n-1] is read through the index, filtered, kept; a second pass in file order walks each read's CIGAR along the loci
// it covers.  Only names that occur more than once among the entered reads need the per-locus memory of "the first read of this name".
namespace cto {

int allele_counts_host_range(const char* bam_path, const char* bai_path, const char* ctg_name, const int32_t* loci, int64_t n_loci,
                             const AlleleParams& pr, int32_t* counts, int64_t* n_entered, double* ms_records, double* ms_count) {
    const double t0 = now();
    memset(counts, 0, size_t(n_loci) * 4 * sizeof(int32_t));
    BamRegion rg;
    CTO_REQUIRE(rg.open("cto_allele_counts", bam_path, bai_path, ctg_name, int64_t(loci[0]) - 1, loci[n_loci - 1], false, false), CTO_EINVAL, "%s",
                rg.err.c_str());
    struct ARead {
        int32_t pos, end, l_seq;
        int name_id;
        size_t seq_off, qual_off;
        std::vector<uint32_t> cigar;
        std::vector<uint8_t> raw;
    };
    std::vector<ARead> reads;
    std::unordered_map<std::string, int> name_ids;
    std::vector<int> name_uses;
    for (BamRecord b;;) {
        const int got = rg.next(&b);
        CTO_REQUIRE(got >= 0, CTO_EINVAL, "%s", rg.err.c_str());
        if (got == 0) break;
        const int flag = b.flag;
        if (b.mapq < pr.min_mq || (flag & pr.excl_flags) || (flag & pr.req_flags) != pr.req_flags) continue;
        if ((pr.req_flags & 2) && (((flag & 32) != 0) == ((flag & 16) != 0))) continue;     // proper pairs must be F/R
        if ((flag & 1796) || b.n_cig == 0 || b.l_seq <= 0 || b.pos < 0) continue;           // the pile-up iterator's own mask
        CTO_REQUIRE(rg.lay_out(&b), CTO_EINVAL, "%s", rg.err.c_str());
        const int enters = rg.enters(b);
        CTO_REQUIRE(enters >= 0, CTO_EINVAL, "%s", rg.err.c_str());
        if (!enters) continue;
        ARead r;
        r.cigar.resize(size_t(b.n_ops));
        for (int i = 0; i < b.n_ops; ++i) r.cigar[size_t(i)] = b.op(i);
        r.pos = b.pos;
        r.end = int32_t(b.pos + b.rlen);
        r.l_seq = b.l_seq;
        r.seq_off = size_t(b.sq - rg.rec.data());
        r.qual_off = size_t(b.ql - rg.rec.data());
        const auto it = name_ids.emplace(std::string(reinterpret_cast<const char*>(b.name), size_t(std::max(0, b.l_name - 1))), int(name_uses.size()));
        if (it.second) name_uses.push_back(0);
        r.name_id = it.first->second;
        ++name_uses[size_t(r.name_id)];
        r.raw.swap(rg.rec);
        reads.push_back(std::move(r));
    }
    const double t1 = now();
    // (locus index, name) -> base code of the first read of that name that covers the locus
    std::unordered_map<uint64_t, uint8_t> first_c;
    for (const ARead& r : reads) {
        const bool shared_name = name_uses[size_t(r.name_id)] > 1;
        int64_t li = std::lower_bound(loci, loci + n_loci, r.pos + 1) - loci;          // loci are 1-based
        int32_t rp = r.pos, qp = 0;
        for (size_t k = 0; k < r.cigar.size() && li < n_loci && loci[li] <= r.end; ++k) {
            const int len = int(r.cigar[k] >> 4), opc = int(r.cigar[k] & 15);
            const bool cons_ref = consumes_ref(opc);
            const bool cons_q = consumes_query(opc);
            if (cons_ref) {
                const bool is_del = opc == 2 || opc == 3;
                for (; li < n_loci && int64_t(loci[li]) - 1 < int64_t(rp) + len; ++li) {
                    const int q = is_del ? qp : qp + (loci[li] - 1 - rp);
                    const int c = q < r.l_seq ? (r.raw[r.seq_off + size_t(q >> 1)] >> ((~q & 1) << 2)) & 15 : 0;
                    const int bq = q < r.l_seq ? int(r.raw[r.qual_off + size_t(q)]) : 0;
                    bool counts_here = !is_del && bq >= pr.min_bq;
                    if (shared_name) {
                        const auto ins = first_c.emplace((uint64_t(li) << 32) | uint32_t(r.name_id), uint8_t(c));
                        if (!ins.second && int(ins.first->second) == c) counts_here = false;
                    }
                    if (counts_here) {
                        const int slot = c == 1 ? 0 : (c == 2 ? 1 : (c == 4 ? 2 : (c == 8 ? 3 : -1)));
                        if (slot >= 0) ++counts[li * 4 + slot];
                    }
                }
                rp += len;
            }
            if (cons_q) qp += len;
        }
    }
    if (n_entered) *n_entered = int64_t(reads.size());
    if (ms_records) *ms_records = t1 - t0;
    if (ms_count) *ms_count = now() - t1;
    return CTO_OK;
}

// Cuts a contig's loci into chunks whose inflated alignment bytes are expected to stay within `budget`: the linear index names, per
// 16 kb window, the file offset of the first alignment that overlaps it, so the compressed bytes between two positions are read off it
// (interpolated inside a window) and taken times four, the usual ratio of a BAM.  cuts = chunk boundaries as loci indices, 0 .. n_loci.
int allele_plan_chunks(const char* bam_path, const char* bai_path, const char* ctg_name, const int32_t* loci, int64_t n_loci, int64_t budget,
                       std::vector<int64_t>* cuts) {
    cuts->assign(1, 0);
    BamRegion rg;
    CTO_REQUIRE(rg.open("cto_allele_counts", bam_path, bai_path, ctg_name, int64_t(loci[0]) - 1, loci[n_loci - 1], true, false), CTO_EINVAL, "%s",
                rg.err.c_str());
    if (rg.chunks.empty() || rg.linear.empty()) { cuts->push_back(n_loci); return CTO_OK; }
    int64_t file_lo = int64_t(rg.chunks.front().beg >> 16), file_hi = 0;
    for (const Chunk& c : rg.chunks) file_hi = std::max<int64_t>(file_hi, int64_t(c.end >> 16) + 65536);
    std::vector<int64_t> woff(rg.linear.size() + 1);
    for (size_t w = 0; w < rg.linear.size(); ++w) {
        int64_t v = int64_t(rg.linear[w] >> 16);
        if (v == 0) v = w ? woff[w - 1] : file_lo;                  // a window without alignments
        v = std::min(std::max(v, file_lo), file_hi);
        woff[w] = w ? std::max(v, woff[w - 1]) : v;
    }
    woff[rg.linear.size()] = file_hi;
    auto at = [&](int64_t p0) -> double {
        const int64_t w = p0 >> 14;
        if (w >= int64_t(rg.linear.size())) return double(file_hi);
        return double(woff[size_t(w)]) + double(woff[size_t(w) + 1] - woff[size_t(w)]) * double(p0 & 16383) / 16384.0;
    };
    int64_t s = 0;
    for (int64_t i = 1; i < n_loci; ++i)
        if (4.0 * (at(loci[i]) - at(loci[s] - 1)) > double(budget)) { cuts->push_back(i); s = i; }
    cuts->push_back(n_loci);
    return CTO_OK;
}

// ------------------------------------------------------------------------------------------------ AF tallies, host path
// The plain definition of the AF-tally rules (listed in full at the top of csrc/aftally.hip, which holds the C entry point and the
// device path that is held equal to this one).  Every read that overlaps ctg:first-last selected locus is read through the index and
// filtered as the column pile-up above filters; the reads are then walked in file order, so that per locus
//   cover    counts the entered reads over it, reference skips included - the reads behind the first max_depth are not looked at;
//   depth    counts the entries (an aligned base with its indel suffix, or the `*` of a deletion);
//   the HP values of the covers queue up and entry i takes the i-th of them, as zip(base_list, hp_values) pairs them.
int af_tallies_host_range(const char* bam_path, const char* bai_path, const char* ctg_name, const AfLoci& L, const int64_t* sel, int64_t n_sel,
                          const AfParams& pr, int32_t* out, int64_t* n_entered, double* ms_records, double* ms_count) {
    const double t0 = now();
    if (n_entered) *n_entered = 0;
    if (n_sel <= 0) return CTO_OK;
    std::vector<int32_t> pos(static_cast<size_t>(n_sel));           // 1-based, ascending
    for (int64_t i = 0; i < n_sel; ++i) {
        pos[size_t(i)] = L.pos[sel[i]];
        memset(out + sel[i] * 8, 0, 8 * sizeof(int32_t));
    }
    BamRegion rg;
    CTO_REQUIRE(rg.open("cto_af_tallies", bam_path, bai_path, ctg_name, int64_t(pos.front()) - 1, pos.back(), false, false), CTO_EINVAL, "%s",
                rg.err.c_str());
    std::vector<int32_t> cover(size_t(n_sel), 0);
    std::vector<std::vector<uint8_t>> hpq(pr.with_hp ? size_t(n_sel) : 0);      // HP classes of the covers no entry has taken yet
    std::vector<uint32_t> hpq_head(pr.with_hp ? size_t(n_sel) : 0, 0);
    int64_t entered = 0;
    double t_count = 0.0;
    for (BamRecord b;;) {
        const int got = rg.next(&b);
        CTO_REQUIRE(got >= 0, CTO_EINVAL, "%s", rg.err.c_str());
        if (got == 0) break;
        const int flag = b.flag;
        if ((flag & pr.excl_flags) || (flag & 4) || b.mapq < pr.min_mq || b.n_cig == 0 || b.l_seq <= 0 || b.pos < 0) continue;
        if ((flag & 1) && !(flag & 2)) continue;           // orphan (mpileup without -A)
        CTO_REQUIRE(rg.lay_out(&b), CTO_EINVAL, "%s", rg.err.c_str());
        const int enters = rg.enters(b);
        CTO_REQUIRE(enters >= 0, CTO_EINVAL, "%s", rg.err.c_str());
        if (!enters) continue;
        ++entered;
        const double tc0 = now();
        int hp = 0;                                        // 0, 1, 2; 3 = the value 12, which the reference cannot index with
        if (pr.with_hp) {
            const uint8_t* aux = b.aux;
            long long val;
            for (AuxField f; aux_next(&aux, b.end, &f);)
                if (f.t0 == 'H' && f.t1 == 'P' && aux_int(f, &val)) { hp = val == 1 ? 1 : (val == 2 ? 2 : (val == 12 ? 3 : 0)); break; }
        }
        auto base4 = [&](int q) { return (b.sq[q >> 1] >> ((~q & 1) << 2)) & 15; };
        int64_t li = std::lower_bound(pos.begin(), pos.end(), b.pos + 1) - pos.begin();
        int32_t rp = b.pos, qp = 0;
        for (int k = 0; k < b.n_ops && li < n_sel; ++k) {
            const int len = int(b.op(k) >> 4), opc = int(b.op(k) & 15);
            const bool cons_ref = consumes_ref(opc);
            const bool cons_q = consumes_query(opc);
            if (cons_ref) {
                for (; li < n_sel && int64_t(pos[size_t(li)]) - 1 < int64_t(rp) + len; ++li) {
                    const size_t i = size_t(li);
                    const int64_t g = sel[li];
                    int32_t* o = out + g * 8;
                    if (pr.max_depth > 0 && cover[i] >= pr.max_depth) continue;
                    ++cover[i];
                    if (pr.with_hp) hpq[i].push_back(uint8_t(hp));
                    if (opc == 3) continue;                // N: an HP value, no entry
                    bool match = false;
                    if (opc != 2) {                        // an aligned base; D is the entry `*`, which no allele equals
                        const int off = pos[i] - 1 - rp, q = qp + off;
                        const int c = base4(q);
                        const char letter = c == 1 ? 'A' : (c == 2 ? 'C' : (c == 4 ? 'G' : (c == 8 ? 'T' : 'N')));
                        int suffix = 0, nlen = 0;          // 1: +SEQ, 2: -N..N
                        if (off == len - 1) {
                            int nx = k + 1;
                            while (nx < b.n_ops && (b.op(nx) & 15) == 6) ++nx;      // P
                            if (nx < b.n_ops && ((b.op(nx) & 15) == 1 || (b.op(nx) & 15) == 2)) { suffix = int(b.op(nx) & 15); nlen = int(b.op(nx) >> 4); }
                        }
                        const int kind = L.kind[g];
                        if (char(L.base[g]) == letter) {
                            if (kind == 0) match = suffix == 0;
                            else if (kind == 2) match = suffix == 2 && nlen == L.del_len[g];
                            else if (kind == 1 && suffix == 1 && int64_t(nlen) == L.ins_off[g + 1] - L.ins_off[g]) {
                                const char* want = L.ins_bytes + L.ins_off[g];
                                match = true;
                                for (int x = 0; x < nlen && match; ++x) {
                                    char ib = kNt16[base4(q + 1 + x)];
                                    if (ib == '=') ib = 'N';
                                    match = ib == want[x];
                                }
                            }
                        }
                    }
                    ++o[0];
                    o[1] += match;
                    if (pr.with_hp) {
                        const int h = hpq[i][hpq_head[i]++];
                        CTO_REQUIRE(h != 3, CTO_EINVAL, "cto_af_tallies: an entry at %s:%d is paired with HP:i:12, which the reference's HAP_LIST[int(hap)] cannot index "
                                    "(src/cal_af_distribution.py:107 raises IndexError)", ctg_name, int(pos[i]));
                        ++o[5 + h];
                        o[2 + h] += match;
                    }
                }
                rp += len;
            }
            if (cons_q) qp += len;
        }
        t_count += now() - tc0;
    }
    if (n_entered) *n_entered = entered;
    if (ms_records) *ms_records = now() - t0 - t_count;
    if (ms_count) *ms_count = t_count;
    return CTO_OK;
}

// ------------------------------------------------------------------------------------------------ read phasing, host path
// The plain definition of the phasing rules (listed in full at the top of csrc/phase.hip, which holds the C entry point and the device
// path that is held equal to this one): observations per chunk of sites, their merge by virtual offset, the link table, the sequential
// phase pass (which both paths run here) and the reads' haplotypes.

// The observations of the sites [a, b) by every read that enters their stretch [pos[a] - 1, pos[b] - 1) - the stretches of a call's
// chunks tile pos[0] - 1 .. pos[n - 1], so a read enters at least one chunk exactly when it enters the whole.
int phase_observe_host_range(const char* bam_path, const char* bai_path, const char* ctg_name, const PhaseSites& S, int64_t a, int64_t b,
                             const PhaseParams& pr, PhaseReads* out, double* ms) {
    const double t0 = now();
    out->voff.clear(); out->obs.clear(); out->off.assign(1, 0);
    const int64_t beg0 = int64_t(S.pos[a]) - 1, end0 = b < S.n ? int64_t(S.pos[b]) - 1 : int64_t(S.pos[S.n - 1]);
    BamRegion rg;
    CTO_REQUIRE(rg.open("cto_phase_reads", bam_path, bai_path, ctg_name, beg0, end0, false, false), CTO_EINVAL, "%s", rg.err.c_str());
    const int32_t *p0 = S.pos + a, *p1 = S.pos + b;
    for (BamRecord r;;) {
        const int got = rg.next(&r);
        CTO_REQUIRE(got >= 0, CTO_EINVAL, "%s", rg.err.c_str());
        if (got == 0) break;
        const int flag = r.flag;
        if ((flag & pr.excl_flags) || (flag & 4) || r.mapq < pr.min_mq || r.n_cig == 0 || r.l_seq <= 0 || r.pos < 0) continue;
        if ((flag & 1) && !(flag & 2)) continue;
        CTO_REQUIRE(rg.lay_out(&r), CTO_EINVAL, "%s", rg.err.c_str());
        const int enters = rg.enters(r);
        CTO_REQUIRE(enters >= 0, CTO_EINVAL, "%s", rg.err.c_str());
        if (!enters) continue;
        out->voff.push_back(rg.rec_voff);
        int64_t li = a + (std::lower_bound(p0, p1, r.pos + 1) - p0);
        int32_t rp = r.pos, qp = 0;
        for (int k = 0; k < r.n_ops && li < b; ++k) {
            const int len = int(r.op(k) >> 4), opc = int(r.op(k) & 15);
            if (consumes_ref(opc)) {
                for (; li < b && int64_t(S.pos[li]) - 1 < int64_t(rp) + len; ++li) {
                    if (opc != 0 && opc != 7 && opc != 8) continue;                 // D, N: nothing
                    const int q = qp + (S.pos[li] - 1 - rp);
                    const int c = (r.sq[q >> 1] >> ((~q & 1) << 2)) & 15;
                    if (c != 1 && c != 2 && c != 4 && c != 8) continue;             // N, IUPAC codes, `=`: nothing
                    if (c == phase_base_code(S.ref[li])) out->obs.push_back(int32_t(li * 2));
                    else if (c == phase_base_code(S.alt[li])) out->obs.push_back(int32_t(li * 2 + 1));
                }
                rp += len;
            }
            if (consumes_query(opc)) qp += len;
        }
        out->off.push_back(int64_t(out->obs.size()));
    }
    if (ms) *ms = now() - t0;
    return CTO_OK;
}

// The chunks' reads as one list in file order: a read that entered several chunks is one read, its observations in site order
// (chunks ascend, and each site belongs to one chunk)
void phase_merge(const std::vector<PhaseReads>& parts, PhaseReads* out, int64_t* n_merged) {
    struct Key { uint64_t voff; uint32_t part, idx; };
    std::vector<Key> keys;
    for (size_t p = 0; p < parts.size(); ++p)
        for (size_t i = 0; i < parts[p].voff.size(); ++i) keys.push_back(Key{parts[p].voff[i], uint32_t(p), uint32_t(i)});
    std::stable_sort(keys.begin(), keys.end(), [](const Key& x, const Key& y) { return x.voff < y.voff; });
    out->voff.clear(); out->obs.clear(); out->off.assign(1, 0);
    int64_t merged = 0;
    for (size_t k = 0; k < keys.size(); ++k) {
        const bool first = k == 0 || keys[k].voff != keys[k - 1].voff;
        if (first) out->voff.push_back(keys[k].voff);
        else if (k < 2 || keys[k - 2].voff != keys[k].voff) ++merged;
        const PhaseReads& P = parts[keys[k].part];
        out->obs.insert(out->obs.end(), P.obs.begin() + P.off[keys[k].idx], P.obs.begin() + P.off[keys[k].idx + 1]);
        if (first) out->off.push_back(0);
        out->off.back() = int64_t(out->obs.size());
    }
    if (n_merged) *n_merged = merged;
}

void phase_link_host(const PhaseReads& R, int64_t n, int K, int32_t* link) {
    std::fill(link, link + n * K * 2, 0);
    for (size_t r = 0; r + 1 < R.off.size(); ++r)
        for (int64_t i = R.off[r]; i < R.off[r + 1]; ++i)
            for (int64_t j = i + 1; j < R.off[r + 1] && (R.obs[j] >> 1) - (R.obs[i] >> 1) <= K; ++j)
                ++link[((int64_t(R.obs[i] >> 1)) * K + ((R.obs[j] >> 1) - (R.obs[i] >> 1) - 1)) * 2 + ((R.obs[i] ^ R.obs[j]) & 1)];
}

// The phase pass: one scan over the sites, each judged by the link counts to the phased sites of the open block within K in front of it
void phase_sites(const int32_t* link, const int32_t* pos, int64_t n, int K, int8_t* phase, int32_t* ps, int32_t* block, int64_t* n_blocks) {
    int32_t cur = -1, cur_ps = 0;
    for (int64_t b = 0; b < n; ++b) {
        int64_t same = 0, flip = 0;
        for (int64_t a = std::max<int64_t>(0, b - K); a < b && cur >= 0; ++a) {
            if (block[a] != cur) continue;
            const int32_t* l = link + (a * K + (b - a - 1)) * 2;
            same += l[phase[a]];
            flip += l[1 - phase[a]];
        }
        const int64_t T = same + flip;
        if (b == 0 || T < 2) { ++cur; cur_ps = pos[b]; phase[b] = 0; }
        else if (4 * std::min(same, flip) > T) { phase[b] = -1; ps[b] = 0; block[b] = -1; continue; }
        else phase[b] = flip > same;
        block[b] = cur;
        ps[b] = cur_ps;
    }
    if (n_blocks) *n_blocks = cur + 1;
}

void phase_assign_host(const PhaseReads& R, const int8_t* phase, const int32_t* block, const int32_t* ps, uint8_t* hp, int32_t* rps) {
    for (size_t r = 0; r + 1 < R.off.size(); ++r) {
        int best_h1 = 0, best_h2 = 0, best_ps = 0, h1 = 0, h2 = 0, cur = -1, cur_ps = 0;
        auto close = [&] { if (h1 + h2 > best_h1 + best_h2) { best_h1 = h1; best_h2 = h2; best_ps = cur_ps; } };
        for (int64_t i = R.off[r]; i < R.off[r + 1]; ++i) {
            const int s = R.obs[i] >> 1;
            if (phase[s] < 0) continue;
            if (block[s] != cur) { close(); cur = block[s]; cur_ps = ps[s]; h1 = h2 = 0; }
            if (((R.obs[i] & 1) ^ phase[s]) == 0) ++h1; else ++h2;
        }
        close();
        const int t = best_h1 + best_h2;
        hp[r] = t > 0 && 10 * best_h1 >= 6 * t ? 1 : (t > 0 && 10 * best_h2 >= 6 * t ? 2 : 0);
        rps[r] = hp[r] ? best_ps : 0;
    }
}

// ------------------------------------------------------------------------------------------------ haplotype windows, host path
// The plain definition of the rules by which a haplotype-filter job is built from the BAM (listed in full at the top of
// csrc/hapwindows.hip, which holds the C entry point and the device path that is held equal to this one): one pass in file order over
// the reads that overlap the region, each walked along the wanted positions it covers.  Per column two lists grow side by side, as the
// text has them: the COVERS (name, HP, BQ, MQ: one per read over the position that passes --min-BQ, reference skips included) and
// the ENTRIES (base and indel: one per cover that is no skip).  Record i of a column is entry i with cover i's name, HP, BQ and MQ.
int hap_windows_host(const char* bam_path, const char* bai_path, const char* ctg_name, int64_t region_lo, int64_t region_hi, const int64_t* iv,
                     int64_t n_iv, const HapWinParams& pr, HapRaw* raw, int64_t* n_entered) {
    if (n_entered) *n_entered = 0;
    if (n_iv <= 0) return CTO_OK;
    constexpr int32_t NONE = INT32_MIN;
    struct Slot {                                       // cover i and entry i of a column share slot i
        int32_t read; uint8_t bq, mq, base; int32_t indel_off, indel_len, start_idx, end_idx;
    };
    struct ColBuild { std::vector<Slot> s; int32_t n_cov = 0, n_ent = 0; };
    std::vector<int64_t> base(size_t(n_iv) + 1, 0);
    for (int64_t k = 0; k < n_iv; ++k) base[size_t(k) + 1] = base[size_t(k)] + (iv[2 * k + 1] - iv[2 * k]);
    std::vector<ColBuild> cols(static_cast<size_t>(base[size_t(n_iv)]));
    // the depth cap looks at every read of the region in front of the one it judges, so with a cap the pass starts at the region's start
    const int64_t beg0 = pr.max_depth > 0 ? region_lo - 1 : std::max<int64_t>(region_lo - 1, iv[0]);
    const int64_t end0 = std::min<int64_t>(region_hi, iv[2 * n_iv - 1]);
    if (end0 <= beg0) return CTO_OK;
    BamRegion rg;
    CTO_REQUIRE(rg.open("cto_hap_windows", bam_path, bai_path, ctg_name, beg0, end0, false, false), CTO_EINVAL, "%s", rg.err.c_str());
    std::vector<int32_t> live;                          // ends of the accepted reads still open (kept only under a cap)
    int64_t entered = 0;
    for (BamRecord b;;) {
        const int got = rg.next(&b);
        CTO_REQUIRE(got >= 0, CTO_EINVAL, "%s", rg.err.c_str());
        if (got == 0) break;
        const int flag = b.flag;
        if ((flag & pr.excl_flags) || (flag & 4) || b.mapq < pr.min_mq || b.n_cig == 0 || b.l_seq <= 0 || b.pos < 0) continue;
        if ((flag & 1) && !(flag & 2)) continue;           // orphan (mpileup without -A)
        CTO_REQUIRE(rg.lay_out(&b), CTO_EINVAL, "%s", rg.err.c_str());
        const int enters = rg.enters(b);
        CTO_REQUIRE(enters >= 0, CTO_EINVAL, "%s", rg.err.c_str());
        if (!enters) continue;
        const int32_t rend = int32_t(b.pos + b.rlen);
        if (pr.max_depth > 0) {
            live.erase(std::remove_if(live.begin(), live.end(), [&](int32_t e) { return e <= b.pos; }), live.end());
            if (int64_t(live.size()) >= pr.max_depth) continue;
            live.push_back(rend);
        }
        ++entered;
        // first wanted interval that ends behind the read's start
        int64_t kiv = 0;
        for (int64_t z = n_iv; kiv < z;) { const int64_t m = (kiv + z) >> 1; if (iv[2 * m + 1] > b.pos) z = m; else kiv = m + 1; }
        if (kiv >= n_iv || iv[2 * kiv] >= rend) continue;
        const bool rev = (flag & 16) != 0, no_qual = b.ql[0] == 0xff;
        const uint8_t mq = uint8_t(std::min(b.mapq, 93));
        auto base4 = [&](int q) { return (b.sq[q >> 1] >> ((~q & 1) << 2)) & 15; };
        auto bq_at = [&](int q) { return (no_qual || q >= b.l_seq) ? 0 : std::min(int(b.ql[q]), 93); };
        int32_t ridx = -1;
        int32_t rp = b.pos, qp = 0;
        for (int k = 0; k < b.n_ops && kiv < n_iv; ++k) {
            const int len = int(b.op(k) >> 4), opc = int(b.op(k) & 15);
            const bool cons_ref = consumes_ref(opc), cons_q = consumes_query(opc);
            if (cons_ref) {
                const int64_t op_end = int64_t(rp) + len;
                while (kiv < n_iv && iv[2 * kiv] < op_end) {
                    const int64_t s = iv[2 * kiv], e = iv[2 * kiv + 1];
                    for (int64_t p = std::max<int64_t>(rp, s); p < std::min(op_end, e); ++p) {
                        const bool placeholder = opc == 2 || opc == 3;
                        const int q = placeholder ? qp : qp + int(p - rp);      // a deletion or skip: the query base that follows it
                        const int bqv = bq_at(q);
                        if (bqv < pr.min_bq) continue;     // prints nothing: base, ^ and $, quality, name and HP go together
                        if (ridx < 0) {
                            ridx = int32_t(raw->names.size());
                            raw->names.emplace_back(reinterpret_cast<const char*>(b.name), size_t(std::max(0, b.l_name - 1)));
                            int hp = 0;
                            const uint8_t* aux = b.aux;
                            long long val;
                            for (AuxField f; aux_next(&aux, b.end, &f);)
                                if (f.t0 == 'H' && f.t1 == 'P' && aux_int(f, &val)) { hp = val == 1 ? 1 : (val == 2 ? 2 : (val == 12 ? 3 : 0)); break; }
                            raw->hp.push_back(uint8_t(hp));
                        }
                        ColBuild& c = cols[size_t(base[size_t(kiv)] + (p - s))];
                        const int32_t ci = c.n_cov++;
                        if (size_t(ci) == c.s.size()) c.s.push_back(Slot{});
                        c.s[size_t(ci)].read = ridx;
                        c.s[size_t(ci)].bq = uint8_t(bqv);
                        c.s[size_t(ci)].mq = mq;
                        c.s[size_t(ci)].start_idx = p == b.pos ? c.n_ent - 1 : NONE;       // ^ stands in front of the base: the record before it
                        if (opc != 3) {
                            Slot& en = c.s[size_t(c.n_ent++)];
                            en.indel_off = en.indel_len = 0;
                            if (opc == 2) en.base = uint8_t(rev && pr.reverse_del ? '#' : '*');
                            else {
                                const int c4 = base4(q);
                                const char letter = c4 == 1 ? 'A' : (c4 == 2 ? 'C' : (c4 == 4 ? 'G' : (c4 == 8 ? 'T' : 'N')));
                                en.base = uint8_t(rev ? letter + 32 : letter);
                                if (p == op_end - 1) {         // the operation's last base: does an indel follow?
                                    int nx = k + 1;
                                    while (nx < b.n_ops && (b.op(nx) & 15) == 6) ++nx;      // P
                                    const int nop = nx < b.n_ops ? int(b.op(nx) & 15) : -1, nlen = nx < b.n_ops ? int(b.op(nx) >> 4) : 0;
                                    if (nop == 1 || nop == 2) {
                                        en.indel_off = int32_t(raw->indel.size());
                                        en.indel_len = nlen + 1;
                                        raw->indel.push_back(nop == 1 ? '+' : '-');
                                        for (int x = 0; x < nlen; ++x) {
                                            char ib = 'N';
                                            if (nop == 1) { ib = kNt16[base4(q + 1 + x)]; if (ib == '=') ib = 'N'; }
                                            raw->indel.push_back(rev ? char(ib + 32) : ib);
                                        }
                                    }
                                }
                            }
                        }
                        c.s[size_t(ci)].end_idx = p == rend - 1 ? c.n_ent - 1 : NONE;       // $ stands behind it
                    }
                    if (e <= op_end) ++kiv; else break;
                }
                rp += len;
            }
            if (cons_q) qp += len;
        }
    }
    // the columns that hold a record (one with covers but no entry is left out: see csrc/hapwindows.hip)
    std::vector<int32_t> starts, ends;
    for (int64_t k = 0; k < n_iv; ++k)
        for (int64_t p = iv[2 * k]; p < iv[2 * k + 1]; ++p) {
            const ColBuild& c = cols[size_t(base[size_t(k)] + (p - iv[2 * k]))];
            if (c.n_ent == 0) continue;
            starts.clear();
            ends.clear();
            for (int32_t i = 0; i < c.n_cov; ++i) {
                const Slot& s = c.s[size_t(i)];
                if (s.start_idx != NONE) starts.push_back(s.start_idx);
                if (s.end_idx != NONE) ends.push_back(s.end_idx);
                if (i < c.n_ent) raw->recs.push_back(HapRawRec{s.read, s.base, s.bq, s.mq, 0, s.indel_off, s.indel_len});
            }
            auto uniq = [](std::vector<int32_t>& v) { std::sort(v.begin(), v.end()); v.erase(std::unique(v.begin(), v.end()), v.end()); };
            uniq(starts);
            uniq(ends);
            const std::vector<int32_t>& win = starts.size() > ends.size() ? starts : ends;
            raw->rse.insert(raw->rse.end(), win.begin(), win.end());
            raw->col_pos.push_back(p + 1);
            raw->col_off.push_back(int64_t(raw->recs.size()));
            raw->rse_off.push_back(int64_t(raw->rse.size()));
        }
    if (n_entered) *n_entered = entered;
    return CTO_OK;
}

// ------------------------------------------------------------------------------------------------ coverage, subsample and merge, host path
// The plain definition of the rules listed at the top of csrc/contam.hip (which holds the C entry points and the device path that is
// held equal to this one), window by window, and the writer of the output BAM and its index.

int contam_read_header(const char* who, const char* bam_path, BamHeader* out) {
    Bgzf bz;
    CTO_REQUIRE(bz.open(bam_path), CTO_EINVAL, "%s: %s", who, bz.err.c_str());
    std::vector<uint8_t>& raw = out->raw;
    raw.assign(8, 0);
    CTO_REQUIRE(bz.read(raw.data(), 8) && memcmp(raw.data(), "BAM\1", 4) == 0, CTO_EINVAL, "%s: %s is not a BAM file%s%s", who, bam_path,
                bz.err.empty() ? "" : ": ", bz.err.c_str());
    const int l_text = le32(raw.data() + 4);
    CTO_REQUIRE(l_text >= 0 && l_text <= (1 << 28), CTO_EINVAL, "%s: %s: bad header text length", who, bam_path);
    raw.resize(size_t(8) + size_t(l_text) + 4);
    CTO_REQUIRE(bz.read(raw.data() + 8, size_t(l_text) + 4), CTO_EINVAL, "%s: %s: truncated header", who, bam_path);
    const int n_ref = le32(raw.data() + 8 + size_t(l_text));
    CTO_REQUIRE(n_ref >= 0, CTO_EINVAL, "%s: %s: bad reference count", who, bam_path);
    for (int r = 0; r < n_ref; ++r) {
        uint8_t h4[4];
        CTO_REQUIRE(bz.read(h4, 4) && le32(h4) > 0 && le32(h4) <= 65536, CTO_EINVAL, "%s: %s: bad reference list", who, bam_path);
        const size_t l_name = size_t(le32(h4)), at = raw.size();
        raw.resize(at + 4 + l_name + 4);
        memcpy(raw.data() + at, h4, 4);
        CTO_REQUIRE(bz.read(raw.data() + at + 4, l_name + 4), CTO_EINVAL, "%s: %s: truncated reference list", who, bam_path);
        const char* nm = reinterpret_cast<const char*>(raw.data() + at + 4);
        out->names.emplace_back(nm, strnlen(nm, l_name));
        out->lens.push_back(int64_t(le32(raw.data() + at + 4 + l_name)));
    }
    return CTO_OK;
}

int contam_plan_windows(const char* who, const char* const* bams, const char* const* bais, int n_src, const char* ctg_name, int64_t L,
                        int64_t budget, std::vector<int64_t>* cuts) {
    const int64_t nw = (L + kContamWindow - 1) / kContamWindow;
    cuts->assign(1, 0);
    if (nw == 0) return CTO_OK;
    std::vector<int64_t> bytes(size_t(nw) + 1, 0);                   // compressed bytes of all sources in front of window w
    for (int s = 0; s < n_src; ++s) {
        BamRegion rg;
        CTO_REQUIRE(rg.open(who, bams[s], bais[s], ctg_name, 0, L, true, false), CTO_EINVAL, "%s", rg.err.c_str());
        if (rg.chunks.empty() || rg.linear.empty()) continue;
        int64_t file_lo = int64_t(rg.chunks.front().beg >> 16), file_hi = 0;
        for (const Chunk& c : rg.chunks) file_hi = std::max<int64_t>(file_hi, int64_t(c.end >> 16) + 65536);
        int64_t prev = file_lo;
        for (int64_t w = 0; w <= nw; ++w) {
            int64_t v = file_hi;
            if (w < int64_t(rg.linear.size())) {
                v = int64_t(rg.linear[size_t(w)] >> 16);
                if (v == 0) v = prev;                                // a window without alignments
                v = std::max(std::min(std::max(v, file_lo), file_hi), prev);
            }
            bytes[size_t(w)] += v - file_lo;
            prev = v;
        }
    }
    int64_t a = 0;
    for (int64_t w = 1; w < nw; ++w)
        if (4 * (bytes[size_t(w) + 1] - bytes[size_t(a)]) + (w + 1 - a) > budget || w + 1 - a > kContamMaxWindows) { cuts->push_back(w); a = w; }
    cuts->push_back(nw);
    return CTO_OK;
}

int cov_window_host(const char* bam_path, const char* bai_path, const char* ctg_name, int64_t w0, int64_t w1, int64_t L, std::vector<int32_t>* carry,
                    int64_t* bases, int32_t* mn, int32_t* mx, int64_t* n_counted) {
    const int64_t e1 = std::min(w1, L), n = e1 - w0;                 // the window's positions inside the contig: [w0, e1)
    std::vector<int32_t> diff(size_t(n) + 1, 0), open;
    int64_t b = 0, counted = 0;
    int32_t depth = int32_t(carry->size());
    for (int32_t e : *carry) {
        if (e < e1) --diff[size_t(e - w0)];
        b += std::min<int64_t>(e, e1) - w0;
        if (e > e1) open.push_back(e);
    }
    BamRegion rg;
    CTO_REQUIRE(rg.open("cto_bam_coverage", bam_path, bai_path, ctg_name, w0, e1, false, false), CTO_EINVAL, "%s", rg.err.c_str());
    for (BamRecord r;;) {
        const int got = rg.next(&r);
        CTO_REQUIRE(got >= 0, CTO_EINVAL, "%s", rg.err.c_str());
        if (got == 0) break;
        if (r.pos < w0 || (r.flag & kCovExclFlags)) continue;         // an earlier window's, or filtered
        CTO_REQUIRE(rg.lay_out(&r), CTO_EINVAL, "%s", rg.err.c_str());
        const int64_t end = std::min<int64_t>(int64_t(r.pos) + r.rlen, L);
        if (end <= r.pos) continue;
        ++counted;
        ++diff[size_t(r.pos - w0)];
        if (end < e1) --diff[size_t(end - w0)];
        b += std::min(end, e1) - r.pos;
        if (end > e1) open.push_back(int32_t(end));
    }
    int32_t lo = INT32_MAX, hi = INT32_MIN;
    for (int64_t p = 0; p < n; ++p) {
        depth += diff[size_t(p)];
        lo = std::min(lo, depth);
        hi = std::max(hi, depth);
    }
    carry->swap(open);
    *bases = b; *mn = lo; *mx = hi;
    if (n_counted) *n_counted = counted;
    return CTO_OK;
}

int mix_window_host(const char* const* bams, const char* const* bais, const char* ctg_name, int64_t w0, int64_t w1, const int* m, uint32_t seed,
                    std::vector<uint8_t>* stream, std::vector<MixRow>* rows, MixCounts* counts) {
    struct Kept { int32_t pos; std::vector<uint8_t> rec; };
    std::vector<Kept> kept[2];
    *counts = MixCounts{};
    for (int s = 0; s < 2; ++s) {
        BamRegion rg;
        CTO_REQUIRE(rg.open("cto_bam_mix", bams[s], bais[s], ctg_name, w0, w1, false, false), CTO_EINVAL, "%s", rg.err.c_str());
        bool have = false;
        int prev = 0;
        for (BamRecord r;;) {
            const int got = rg.next(&r);
            CTO_REQUIRE(got >= 0, CTO_EINVAL, "%s", rg.err.c_str());
            if (got == 0) break;
            CTO_REQUIRE(!(have && r.pos < prev), CTO_EINVAL, "cto_bam_mix: %s is not coordinate-sorted: position %d of %s behind %d", bams[s],
                        r.pos + 1, ctg_name, prev + 1);
            have = true;
            prev = r.pos;
            if (r.pos < w0) continue;
            CTO_REQUIRE(size_t(32) + size_t(r.l_name) + size_t(r.n_cig) * 4 <= rg.rec.size(), CTO_EINVAL,
                        "cto_bam_mix: alignment record shorter than its fields");
            ++counts->cand[s];
            if (!subsample_keeps(subsample_key(rg.rec.data() + 32, std::max(0, r.l_name - 1), seed), m[s])) continue;
            ++counts->kept[s];
            kept[s].push_back(Kept{r.pos, rg.rec});
        }
    }
    stream->clear();
    rows->clear();
    size_t i = 0, j = 0;
    while (i < kept[0].size() || j < kept[1].size()) {
        const bool tumour = j == kept[1].size() || (i < kept[0].size() && kept[0][i].pos <= kept[1][j].pos);     // equal positions: tumour first
        const Kept& k = tumour ? kept[0][i++] : kept[1][j++];
        const uint8_t* b = k.rec.data();
        const int l_name = b[8], n_cig = b[12] | (b[13] << 8);
        int64_t rlen = 0;
        for (int c = 0; c < n_cig; ++c) {
            const uint32_t op = uint32_t(le32(b + 32 + l_name + size_t(c) * 4));
            if (consumes_ref(int(op & 15))) rlen += int64_t(op >> 4);
        }
        rows->push_back(MixRow{k.pos, int32_t(std::min<int64_t>(rlen, INT32_MAX)), b[10] | (b[11] << 8), 0, int64_t(stream->size())});
        const uint32_t bsz = uint32_t(k.rec.size());
        const uint8_t h4[4] = {uint8_t(bsz), uint8_t(bsz >> 8), uint8_t(bsz >> 16), uint8_t(bsz >> 24)};
        stream->insert(stream->end(), h4, h4 + 4);
        stream->insert(stream->end(), k.rec.begin(), k.rec.end());
    }
    return CTO_OK;
}

namespace {
constexpr size_t kBgzfPayload = 0xff00;
// one BGZF block of data[0 .. n) at zlib level 6, stored when the deflated bytes would not fit; false when zlib fails
bool bgzf_block(z_stream* zs, z_stream* zs0, const uint8_t* data, size_t n, std::vector<uint8_t>* out) {
    out->resize(18 + 65536 + 8);
    size_t clen = 0;
    for (z_stream* z : {zs, zs0}) {
        deflateReset(z);
        z->next_in = const_cast<uint8_t*>(data);
        z->avail_in = uInt(n);
        z->next_out = out->data() + 18;
        z->avail_out = 65536;
        const int rc = deflate(z, Z_FINISH);
        clen = 65536 - z->avail_out;
        if (rc == Z_STREAM_END && clen + 26 <= 65536) break;
        if (z == zs0) return false;
    }
    uint8_t* h = out->data();
    const uint8_t head[16] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0};
    memcpy(h, head, 16);
    const uint32_t bs = uint32_t(clen + 25), crc = uint32_t(crc32(crc32(0L, Z_NULL, 0), data, uInt(n)));
    h[16] = uint8_t(bs); h[17] = uint8_t(bs >> 8);
    uint8_t* t = h + 18 + clen;
    for (int k = 0; k < 4; ++k) { t[k] = uint8_t(crc >> (8 * k)); t[4 + k] = uint8_t(uint32_t(n) >> (8 * k)); }
    out->resize(18 + clen + 8);
    return true;
}
}  // namespace

int MixWriter::open(const char* out_path, const BamHeader& h, int n_threads, int deflate_mode, void* hip_stream) {
    path = out_path;
    coder = deflate_mode;
    stream = hip_stream;
    n_ref = int(h.names.size());
    threads = std::max(1, std::min(n_threads, 64));
    f = fopen(out_path, "wb");
    CTO_REQUIRE(f, CTO_EINVAL, "cto_bam_mix: cannot write %s", out_path);
    pending = h.raw;
    return CTO_OK;
}

// writes the whole blocks of `pending` (all: the rest too, then the empty end block)
int MixWriter::flush(bool all) {
    const double t0 = now();
    size_t n_blocks = pending.size() / kBgzfPayload;
    if (all && pending.size() % kBgzfPayload) ++n_blocks;
    const size_t n_jobs = n_blocks + (all ? 1 : 0);                 // the end block is a job of no bytes
    std::vector<std::vector<uint8_t>> out(n_jobs);
    std::atomic<size_t> next{0};
    std::atomic<bool> ok{true};
    if (coder == 1 && n_blocks) {                                 // up, csrc/deflate.hip, down
        std::vector<uint8_t> bytes;
        std::vector<uint32_t> sizes;
        const int rc = bgzf_deflate_updown(pending.data(), int64_t(std::min(n_blocks * kBgzfPayload, pending.size())), static_cast<hipStream_t>(stream),
                                           &bytes, &sizes, &dst);
        if (rc != CTO_OK) return rc;
        size_t at = 0;
        for (size_t k = 0; k < n_blocks; ++k) { out[k].assign(bytes.begin() + long(at), bytes.begin() + long(at + sizes[k])); at += sizes[k]; }
        next = n_blocks;
    }
    auto work = [&] {
        if (coder) {                                              // the host restatement (the end block: the same 28 bytes)
            cto::dfl::BlockInfo info;
            for (size_t k; (k = next.fetch_add(1)) < n_jobs;) {
                const size_t at = k * kBgzfPayload, n = k < n_blocks ? std::min(kBgzfPayload, pending.size() - at) : 0;
                out[k].resize(65536);
                out[k].resize(size_t(cto::dfl::encode_block(pending.data() + std::min(at, pending.size()), int(n), out[k].data(), &info)));
                if (k < n_blocks && coder == 2) {
                    static std::mutex mu;
                    std::lock_guard<std::mutex> lock(mu);
                    ++dst.n_blocks;
                    dst.in_bytes += int64_t(n);
                    dst.out_bytes += int64_t(out[k].size());
                    ++(info.type == 0 ? dst.stored : info.type == 1 ? dst.fixed : dst.dynamic);
                }
            }
            return;
        }
        z_stream zs, zs0;
        memset(&zs, 0, sizeof zs);
        memset(&zs0, 0, sizeof zs0);
        if (deflateInit2(&zs, 6, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) { ok = false; return; }
        if (deflateInit2(&zs0, 0, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) { deflateEnd(&zs); ok = false; return; }
        for (size_t k; (k = next.fetch_add(1)) < n_jobs;) {
            const size_t at = k * kBgzfPayload, n = k < n_blocks ? std::min(kBgzfPayload, pending.size() - at) : 0;
            if (!bgzf_block(&zs, &zs0, pending.data() + std::min(at, pending.size()), n, &out[k])) ok = false;
        }
        deflateEnd(&zs);
        deflateEnd(&zs0);
    };
    const size_t nt = std::min<size_t>(size_t(threads), std::max<size_t>(n_jobs, 1));
    if (nt <= 1) work();
    else {
        std::vector<std::thread> th;
        for (size_t t = 0; t < nt; ++t) th.emplace_back(work);
        for (auto& x : th) x.join();
    }
    CTO_REQUIRE(ok.load(), CTO_EINVAL, "cto_bam_mix: deflate failed");
    for (size_t k = 0; k < n_jobs; ++k) {
        if (k < n_blocks) coff.push_back(file_off);
        else end_off = file_off;
        CTO_REQUIRE(fwrite(out[k].data(), 1, out[k].size(), f) == out[k].size(), CTO_EINVAL, "cto_bam_mix: cannot write %s", path.c_str());
        file_off += int64_t(out[k].size());
    }
    const size_t used = std::min(n_blocks * kBgzfPayload, pending.size());
    pending.erase(pending.begin(), pending.begin() + used);
    u_pending += int64_t(used);
    ms += now() - t0;
    return CTO_OK;
}

void MixWriter::add_rows(int tid, size_t n, const MixRow* rows, size_t n_rows) {
    const int64_t base = u_pending + int64_t(pending.size());
    for (size_t i = 0; i < n_rows; ++i) {
        const int64_t u0 = base + rows[i].off, u1 = i + 1 < n_rows ? base + rows[i + 1].off : base + int64_t(n);
        recs.push_back(Rec{tid, rows[i].pos, rows[i].rlen, rows[i].bin, u0, u1});
    }
}

int MixWriter::append(int tid, const uint8_t* stream, size_t n, const MixRow* rows, size_t n_rows) {
    add_rows(tid, n, rows, n_rows);
    pending.insert(pending.end(), stream, stream + n);
    return pending.size() >= kBgzfPayload ? flush(false) : CTO_OK;
}

int MixWriter::append_coded(int tid, size_t n, const MixRow* rows, size_t n_rows, const uint32_t* sizes, size_t n_blocks, const uint8_t* blocks,
                            const uint8_t* rest, size_t n_rest) {
    const double t0 = now();
    CTO_REQUIRE(pending.size() + n == n_blocks * kBgzfPayload + n_rest && n_rest < kBgzfPayload, CTO_EINVAL,
                "cto_bam_mix: %zu coded blocks and %zu bytes for %zu pending and %zu new bytes", n_blocks, n_rest, pending.size(), n);
    add_rows(tid, n, rows, n_rows);
    size_t total = 0;
    for (size_t k = 0; k < n_blocks; ++k) { coff.push_back(file_off + int64_t(total)); total += sizes[k]; }
    CTO_REQUIRE(fwrite(blocks, 1, total, f) == total, CTO_EINVAL, "cto_bam_mix: cannot write %s", path.c_str());
    file_off += int64_t(total);
    u_pending += int64_t(n_blocks * kBgzfPayload);
    pending.assign(rest, rest + n_rest);
    ms += now() - t0;
    return CTO_OK;
}

int MixWriter::close(int64_t* out_bytes, int64_t* out_blocks) {
    const int64_t total = u_pending + int64_t(pending.size());
    int rc = flush(true);
    if (rc != CTO_OK) return rc;
    CTO_REQUIRE(fclose(f) == 0, CTO_EINVAL, "cto_bam_mix: cannot write %s", path.c_str());
    f = nullptr;
    if (out_bytes) *out_bytes = total;
    if (out_blocks) *out_blocks = int64_t(coff.size());
    // the virtual offset of stream byte u, as a writer names it that flushes whenever 0xff00 bytes are pending
    auto voff = [&](int64_t u) -> uint64_t {
        const size_t k = size_t(u / int64_t(kBgzfPayload));
        return (uint64_t(k < coff.size() ? coff[k] : end_off) << 16) | uint64_t(u % int64_t(kBgzfPayload));
    };
    const double t0 = now();
    std::string bai("BAI\1", 4);
    auto put32 = [&](uint32_t v) { for (int k = 0; k < 4; ++k) bai += char(uint8_t(v >> (8 * k))); };
    auto put64 = [&](uint64_t v) { put32(uint32_t(v)); put32(uint32_t(v >> 32)); };
    put32(uint32_t(n_ref));
    size_t at = 0;
    for (int t = 0; t < n_ref; ++t) {
        std::map<uint32_t, std::vector<Chunk>> bins;
        std::vector<uint64_t> lin;
        std::vector<bool> lin_set;
        for (; at < recs.size() && recs[at].tid == t; ++at) {
            const Rec& r = recs[at];
            const uint64_t vb = voff(r.u0), ve = voff(r.u1);
            std::vector<Chunk>& ch = bins[uint32_t(r.bin)];
            if (!ch.empty() && ch.back().end == vb) ch.back().end = ve;
            else ch.push_back(Chunk{vb, ve});
            const int64_t beg = std::max(r.pos, 0), end = std::max<int64_t>(beg + 1, int64_t(r.pos) + r.rlen);
            const size_t wl = size_t((end - 1) >> 14);
            if (lin.size() <= wl) { lin.resize(wl + 1, 0); lin_set.resize(wl + 1, false); }
            for (size_t w = size_t(beg >> 14); w <= wl; ++w)
                if (!lin_set[w]) { lin_set[w] = true; lin[w] = vb; }
        }
        put32(uint32_t(bins.size()));
        for (const auto& b : bins) {
            put32(b.first);
            put32(uint32_t(b.second.size()));
            for (const Chunk& c : b.second) { put64(c.beg); put64(c.end); }
        }
        put32(uint32_t(lin.size()));
        uint64_t last = 0;
        for (size_t w = 0; w < lin.size(); ++w) {
            if (lin_set[w]) last = lin[w];
            put64(last);
        }
    }
    const std::string bai_path = path + ".bai";
    FILE* g = fopen(bai_path.c_str(), "wb");
    CTO_REQUIRE(g, CTO_EINVAL, "cto_bam_mix: cannot write %s", bai_path.c_str());
    const bool wrote = fwrite(bai.data(), 1, bai.size(), g) == bai.size();
    CTO_REQUIRE((fclose(g) == 0) && wrote, CTO_EINVAL, "cto_bam_mix: cannot write %s", bai_path.c_str());
    ms += now() - t0;
    return CTO_OK;
}

}  // namespace cto

// The byte range of the BAM that holds every BGZF block the index names for ctg:start-end (the block the last chunk ends in
// included: a BGZF block is at most 64 KiB long).
extern "C" int cto_bam_chunk_span(const char* bam_path, const char* bai_path, const char* ctg_name, int64_t start, int64_t end,
                                   int64_t* file_begin, int64_t* file_end) {
    return guarded("cto_bam_chunk_span", [&] {
        CTO_REQUIRE(bam_path && ctg_name && file_begin && file_end, CTO_EINVAL, "cto_bam_chunk_span: null argument");
        CTO_REQUIRE(start >= 1 && end >= start, CTO_EINVAL, "cto_bam_chunk_span: bad region %lld-%lld", (long long)start, (long long)end);
        BamRegion rg;
        CTO_REQUIRE(rg.open("cto_bam_chunk_span", bam_path, bai_path, ctg_name, start - 1, end, true, false), CTO_EINVAL, "%s", rg.err.c_str());
        const int64_t fsize = rg.bz.fsize;
        int64_t lo = fsize, hi = 0;
        for (const Chunk& c : rg.chunks) {
            lo = std::min<int64_t>(lo, int64_t(c.beg >> 16));
            hi = std::max<int64_t>(hi, int64_t(c.end >> 16) + 65536);
        }
        if (rg.chunks.empty()) { lo = 0; hi = 0; }
        // The chunk lists of the coarse bins (a 512 Mb bin holds every read that straddles a finer boundary) end far behind the
        // region - the reader stops at the first alignment that starts after it, this range has to be cut beforehand.  The file is
        // sorted: the linear index names, per 16 kb window, the first alignment that overlaps it, and once THAT alignment starts
        // after the region everything from its block on does.  A few one-block probes find the window.
        if (!rg.chunks.empty()) {
            const int64_t w0 = ((end - 1) >> 14) + 1;
            uint64_t last = 0;
            int probes = 0;
            for (int64_t w = w0; w < int64_t(rg.linear.size()) && probes < 48; ++w) {
                const uint64_t v = rg.linear[size_t(w)];
                if (v == 0 || v == last || int64_t(v >> 16) < lo) continue;
                last = v;
                ++probes;
                uint8_t head[12];
                if (!rg.bz.seek(v) || !rg.bz.read(head, 12)) break;         // damaged index / file: keep the wide range
                const int32_t rid = le32(head + 4), pos0 = le32(head + 8);
                if (rid != rg.tid || int64_t(pos0) >= end) {             // starts after the region (1-based end = 0-based exclusive end)
                    hi = std::min<int64_t>(hi, int64_t(v >> 16) + 65536);
                    break;
                }
            }
        }
        *file_begin = lo;
        *file_end = std::min(hi, fsize);
        return CTO_OK;
    });
}

// `samtools view BAM ctg:start-end [-q min_mq]` without samtools: the alignments overlapping the region as SAM rows (no header),
// QNAME FLAG RNAME POS MAPQ CIGAR RNEXT PNEXT TLEN SEQ QUAL and, when the record has one, its HP:i tag - what
// src/realign_reads.py:255-300 reads of every row.  Returns the number of rows; *need = bytes of text (CTO_ENOMEM when cap is less).
extern "C" int64_t cto_bam_view(const char* bam_path, const char* bai_path, const char* ctg_name, int64_t start, int64_t end, int min_mq,
                                char* buf, size_t cap, size_t* need) {
    int64_t n_rows = 0;
    const int rc = guarded("cto_bam_view", [&] {
        CTO_REQUIRE(bam_path && ctg_name && need && (buf || cap == 0), CTO_EINVAL, "cto_bam_view: null argument");
        CTO_REQUIRE(start >= 1 && end >= start, CTO_EINVAL, "cto_bam_view: bad region");
        BamRegion rg;                    // with the reference names: RNEXT of a mate on another contig
        CTO_REQUIRE(rg.open("cto_bam_view", bam_path, bai_path, ctg_name, start - 1, end, false, true), CTO_EINVAL, "%s", rg.err.c_str());
        std::string out;
        for (BamRecord b;;) {
            const int got = rg.next(&b);
            CTO_REQUIRE(got >= 0, CTO_EINVAL, "%s", rg.err.c_str());
            if (got == 0) break;
            CTO_REQUIRE(rg.lay_out(&b), CTO_EINVAL, "%s", rg.err.c_str());      // no filter in front: every record up to the region's end
            // (the CIGAR printed is the laid-out one: of a read with more than 65535 operations its CG:B,I tag, as samtools view does)
            if (int64_t(b.pos) + std::max<int64_t>(b.rlen, 1) <= rg.beg0 || b.mapq < min_mq) continue;
            char num[32];
            out.append(reinterpret_cast<const char*>(b.name), size_t(std::max(0, b.l_name - 1)));
            out += '\t'; out += std::to_string(b.flag); out += '\t'; out += ctg_name; out += '\t'; out += std::to_string(b.pos + 1);
            out += '\t'; out += std::to_string(b.mapq); out += '\t';
            if (b.n_ops == 0) out += '*';
            for (int i = 0; i < b.n_ops; ++i) {
                snprintf(num, sizeof(num), "%u%c", b.op(i) >> 4, "MIDNSHP=X???????"[b.op(i) & 15]);
                out += num;
            }
            out += '\t';
            out += b.next_ref < 0 ? "*" : (b.next_ref == rg.tid ? "=" : (size_t(b.next_ref) < rg.names.size() ? rg.names[size_t(b.next_ref)].c_str() : "*"));
            out += '\t'; out += std::to_string(b.next_pos + 1); out += '\t'; out += std::to_string(b.tlen); out += '\t';
            if (b.l_seq == 0) out += '*';
            for (int i = 0; i < b.l_seq; ++i) out += kNt16[(b.sq[i >> 1] >> ((~i & 1) << 2)) & 15];
            out += '\t';
            if (b.l_seq == 0 || b.ql[0] == 0xff) out += '*';
            else for (int i = 0; i < b.l_seq; ++i) out += char(std::min(int(b.ql[i]), 93) + 33);
            const uint8_t* aux = b.aux;                                          // HP:i of the auxiliary fields, of any integer type
            long long val;
            for (AuxField f; aux_next(&aux, b.end, &f);)
                if (f.t0 == 'H' && f.t1 == 'P' && aux_int(f, &val)) { out += "\tHP:i:"; out += std::to_string(val); }
            out += '\n';
            ++n_rows;
        }
        *need = out.size();
        CTO_REQUIRE(out.size() <= cap, CTO_ENOMEM, "cto_bam_view: %zu bytes of text, room for %zu", out.size(), cap);
        if (!out.empty()) memcpy(buf, out.data(), out.size());
        return CTO_OK;
    });
    return rc == CTO_OK ? n_rows : rc;
}

// Record boundaries the index knows inside [file_begin, file_end): the starts of the region's chunks and, per 16 kb window of the
// region, the first alignment that overlaps it (BAI linear index) - virtual offsets, ascending, the first one being where a
// reader of the region starts.  The device pileup (csrc/pileup.hip) walks one chain of records from each of them.
extern "C" int64_t cto_bam_record_starts(const char* bam_path, const char* bai_path, const char* ctg_name, int64_t start, int64_t end,
                                         int64_t file_begin, int64_t file_end, uint64_t* voffs, int64_t cap, int32_t* tid_out) {
    int64_t n_out = 0;
    const int rc = guarded("cto_bam_record_starts", [&] {
        CTO_REQUIRE(bam_path && ctg_name && voffs && cap > 0 && tid_out, CTO_EINVAL, "cto_bam_record_starts: null argument");
        CTO_REQUIRE(start >= 1 && end >= start, CTO_EINVAL, "cto_bam_record_starts: bad region");
        BamRegion rg;
        CTO_REQUIRE(rg.open("cto_bam_record_starts", bam_path, bai_path, ctg_name, start - 1, end, true, false), CTO_EINVAL, "%s", rg.err.c_str());
        *tid_out = rg.tid;
        if (rg.chunks.empty()) return CTO_OK;
        const uint64_t first = rg.chunks.front().beg;
        std::vector<uint64_t> v;
        for (const Chunk& c : rg.chunks) v.push_back(c.beg);
        const int64_t w0 = (start - 1) >> 14, w1 = std::min<int64_t>(int64_t(rg.linear.size()) - 1, (end - 1) >> 14);
        for (int64_t w = w0; w <= w1; ++w)
            if (w >= 0 && rg.linear[size_t(w)] > first) v.push_back(rg.linear[size_t(w)]);
        std::sort(v.begin(), v.end());
        v.erase(std::unique(v.begin(), v.end()), v.end());
        for (uint64_t x : v) {
            const int64_t coff = int64_t(x >> 16);
            if (coff < file_begin || coff >= file_end) continue;
            if (n_out < cap) voffs[n_out] = x;
            ++n_out;
        }
        CTO_REQUIRE(n_out <= cap, CTO_ENOMEM, "cto_bam_record_starts: %lld offsets, room for %lld", (long long)n_out, (long long)cap);
        return CTO_OK;
    });
    return rc == CTO_OK ? n_out : rc;
}

// Block table of a run of whole BGZF blocks (a trailing partial block is left out).
extern "C" int64_t cto_bgzf_scan(const uint8_t* bytes, size_t len, int64_t file_begin, cto_bgzf_block* blocks, int64_t cap, int64_t* out_bytes) {
    if (!bytes || !blocks || !out_bytes) { set_error("cto_bgzf_scan: null argument"); return CTO_EINVAL; }
    size_t o = 0;
    int64_t n = 0, out = 0;
    for (BgzfHeader h; o < len; o += size_t(h.bsize)) {
        const BgzfHeader::Status st = bgzf_header(bytes + o, len - o, &h);
        if (st == BgzfHeader::MORE) break;                      // partial block at the end of the range
        if (st == BgzfHeader::TOO_LARGE) { set_error("cto_bgzf_scan: %s", bgzf_why(st)); return CTO_EINVAL; }
        if (st != BgzfHeader::OK) { set_error("cto_bgzf_scan: %s at byte %zu", bgzf_why(st), o); return CTO_EINVAL; }
        if (n >= cap) { set_error("cto_bgzf_scan: more than %lld blocks", (long long)cap); return CTO_ENOMEM; }
        cto_bgzf_block& b = blocks[n++];
        b.file_off = uint64_t(file_begin) + o;
        b.in_off = o + 12 + size_t(h.xlen);
        b.out_off = uint64_t(out);
        b.csize = uint32_t(h.cdata);
        b.isize = h.isize;
        b.bsize = uint32_t(h.bsize);
        b.crc32 = h.crc32;
        out += (int64_t(h.isize) + CTO_BGZF_SLOT_PAD + 255) / 256 * 256;   // the inflate kernel checks a literal run's output bound once
                                                                           // per 32 input bits: a malformed block may run that far past its isize
    }
    *out_bytes = out;
    return n;
}
