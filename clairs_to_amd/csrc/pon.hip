// Panel-of-normals scan (cto_pon_*, include/clairsto_amd.h): the PoN pass of src/nonsomatic_tagging.py on the device.
//
// A PoN file becomes text in slabs (plain .vcf: read as is; BGZF: cto_bgzf_scan + k_bgzf_inflate, then the 256-byte-aligned slots
// gathered into contiguous text; other gzip: zlib on the host), and every slab goes through three passes:
//   k_line_count / scan_exclusive / k_line_emit   line starts in file order (16 KiB of text per workgroup)
//   k_pon_parse                                   one lane per line: the '#' and strip rules of _parse_pon_line, CHROM / POS / REF / ALT,
//                                                 binary search of POS among the contig's sorted calls, hit bytes by plain stores
// The last, unfinished line of a slab is carried to the front of the next one; so is a BGZF block cut by the slab's end.  Lines the
// device cannot decide exactly go back to the host (cto_pon_host_lines), which parses them with the reference's own rules.
#include <sys/stat.h>
#include <zlib.h>
#include <algorithm>
#include <chrono>
#include <memory>
#include <string>
#include <vector>
#include "hip_buffers.h"
#include "scan.h"
#include "lines.h"
#include "pack_internal.h"
#include "bam_host.h"

using namespace cto;

namespace {

constexpr size_t SLAB_DEFAULT = size_t(32) << 20;      // compressed (or plain) bytes read per slab; CTO_PON_SLAB overrides (tests: many slabs)
constexpr int POS_DIGITS = 18;                         // longer POS strings go to the host (int64 without overflow)

// inflated BGZF slots -> contiguous text: piece p copies slot bytes [src, src + len) to text[dst, dst + len); one workgroup per piece
__global__ __launch_bounds__(256) void k_gather(const uint8_t* __restrict__ slots, const int64_t* __restrict__ piece, uint8_t* __restrict__ text) {
    const int64_t src = piece[3 * blockIdx.x], len = piece[3 * blockIdx.x + 1], dst = piece[3 * blockIdx.x + 2];
    for (int64_t i = threadIdx.x; i < len; i += 256) text[dst + i] = slots[src + i];
}

struct DevCalls {
    const int64_t* pos;        // [n] sorted by (contig, POS)
    const int64_t* ctg_off;    // [n_ctg + 1] each contig's range of calls
    const int64_t* orig;       // [n] index of the call as the caller numbered it
    const int64_t* str_off;    // [2n + 1] REF, first ALT of each call (sorted order)
    const uint8_t* str;
    const int64_t* name_off;   // [n_ctg + 1]
    const uint8_t* names;
    int n_ctg;
};

__device__ __forceinline__ bool is_ws(uint8_t c) { return c == ' ' || (c >= 9 && c <= 13) || (c >= 0x1c && c <= 0x1f); }  // str.strip(), ASCII

__device__ __forceinline__ bool same(const uint8_t* a, int64_t na, const uint8_t* b, int64_t nb) {
    if (na != nb) return false;
    for (int64_t i = 0; i < na; ++i)
        if (a[i] != b[i]) return false;
    return true;
}

// one lane per line k of [0, n_proc): line = text[starts[k], starts[k + 1] or text_end).  counters[0] = lines handed to the host
// (their indices in host_idx, any order), counters[1] = records.  only >= -1: the --ctg_name form (CHROM must equal the only contig's
// name; -1 = that contig has no calls, only the errors of the POS rule matter); only == -2: CHROM must name one of the call contigs.
__global__ __launch_bounds__(256) void k_pon_parse(const uint8_t* __restrict__ text, uint32_t text_end, const uint32_t* __restrict__ starts,
                                                   uint32_t n_lines, uint32_t n_proc, DevCalls cs, int only, const uint8_t* __restrict__ only_name,
                                                   int only_len, int require_allele, uint8_t* __restrict__ hit, uint32_t* __restrict__ host_idx,
                                                   unsigned int* __restrict__ counters) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    bool record = false, to_host = false;
    if (k < n_proc) {
        uint32_t s = starts[k];
        uint32_t e = k + 1 < n_lines ? starts[k + 1] : text_end;
        do {
            if (text[s] == '#') break;
            while (e > s && is_ws(text[e - 1])) --e;
            if (e > s && text[e - 1] >= 0x80) { to_host = true; break; }   // unicode whitespace may strip more
            while (s < e && is_ws(text[s])) ++s;
            if (s == e) break;
            uint32_t f[6];                        // field starts; f[5] = end of field 4 + 1
            int nf = 1;
            f[0] = s;
            bool high = false;
            uint32_t i = s;
            for (; i < e && nf < 5; ++i) {
                const uint8_t c = text[i];
                high |= c >= 0x80;
                if (c == '\t') f[nf++] = i + 1;
            }
            if (nf < 5) break;                    // fewer than five fields
            for (; i < e && text[i] != '\t'; ++i) high |= text[i] >= 0x80;
            f[5] = i + 1;
            if (high) { to_host = true; break; }
            record = true;
            int c = only;
            if (only == -2) {
                c = -1;
                for (int j = 0; j < cs.n_ctg && c < 0; ++j)
                    if (same(text + f[0], int64_t(f[1] - 1 - f[0]), cs.names + cs.name_off[j], cs.name_off[j + 1] - cs.name_off[j])) c = j;
                if (c < 0) break;                 // not a contig of the call set: skipped before int() sees POS
            }
            const int np = int(f[2] - 1 - f[1]);
            int64_t pos = 0;
            bool digits = np >= 1 && np <= POS_DIGITS;
            for (int j = 0; j < np && digits; ++j) {
                const uint8_t d = text[f[1] + j];
                digits = d >= '0' && d <= '9';
                pos = pos * 10 + (d - '0');
            }
            if (!digits) { to_host = true; break; }
            if (only >= -1 && !same(text + f[0], int64_t(f[1] - 1 - f[0]), only_name, only_len)) break;
            if (c < 0) break;
            int64_t lo = cs.ctg_off[c], hi = cs.ctg_off[c + 1];
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (cs.pos[mid] < pos) lo = mid + 1; else hi = mid;
            }
            const uint8_t* ref = text + f[3];
            const int64_t nref = int64_t(f[4] - 1 - f[3]);
            for (int64_t j = lo; j < cs.ctg_off[c + 1] && cs.pos[j] == pos; ++j) {
                bool h = !require_allele;
                if (!h && same(ref, nref, cs.str + cs.str_off[2 * j], cs.str_off[2 * j + 1] - cs.str_off[2 * j])) {
                    const uint8_t* ca = cs.str + cs.str_off[2 * j + 1];
                    const int64_t nca = cs.str_off[2 * j + 2] - cs.str_off[2 * j + 1];
                    uint32_t a = f[4];
                    for (uint32_t t = f[4]; t <= f[5] - 1 && !h; ++t)     // ALT.split(',')
                        if (t == f[5] - 1 || text[t] == ',') {
                            h = same(text + a, int64_t(t - a), ca, nca);
                            a = t + 1;
                        }
                }
                if (h) hit[cs.orig[j]] = 1;
            }
        } while (false);
    }
    if (to_host) host_idx[atomicAdd(&counters[0], 1u)] = k;
    const unsigned long long rec = __ballot(record);
    if ((threadIdx.x & 63) == 0 && rec) atomicAdd(&counters[1], unsigned(__popcll(rec)));
}

bool is_gzip_magic(const uint8_t* p, size_t n) { return n >= 2 && p[0] == 0x1f && p[1] == 0x8b; }
bool is_bgzf_header(const uint8_t* h, size_t n) {      // of a file's first bytes: the block itself is longer than they are
    BgzfHeader bh;
    const BgzfHeader::Status st = bgzf_header(h, n, &bh);
    return st == BgzfHeader::OK || (st == BgzfHeader::MORE && bh.bsize > 0);
}

// a whole gzip file in memory (a .tbi): every member inflated; false when zlib rejects it
bool gunzip_mem(const uint8_t* in, size_t n, std::vector<uint8_t>* out) {
    size_t o = 0;
    while (o < n && is_gzip_magic(in + o, n - o)) {
        z_stream z{};
        if (inflateInit2(&z, 16 + MAX_WBITS) != Z_OK) return false;
        z.next_in = const_cast<Bytef*>(in + o);
        z.avail_in = uInt(std::min<size_t>(n - o, 1u << 30));
        int rc = Z_OK;
        while (rc == Z_OK) {
            const size_t at = out->size();
            out->resize(at + (1 << 16));
            z.next_out = out->data() + at;
            z.avail_out = 1 << 16;
            rc = inflate(&z, Z_NO_FLUSH);
            out->resize(at + (1 << 16) - z.avail_out);
        }
        o += size_t(z.next_in - (in + o));
        inflateEnd(&z);
        if (rc != Z_STREAM_END) return false;
    }
    return o > 0;
}

}  // namespace

struct cto_pon {
    // call set (sorted by contig, POS)
    int n_ctg = 0;
    int64_t n_calls = 0;
    std::vector<std::string> names;
    DevBuf pos, ctg_off, orig, str_off, str, name_off, name_bytes, only_name;
    // per file
    DevBuf hit, comp, blocks, status, slots, text[2], tiles, tile_base, tile_tmp, tile_tot, starts, host_idx, counters, pieces;
    PinBuf h_in, h_small;
    std::vector<cto_bgzf_block> h_blocks;
    std::vector<int64_t> h_pieces;
    Event ev;
    size_t slab_in = SLAB_DEFAULT, text_cap = 4 * SLAB_DEFAULT;   // inflated bytes per slab, at most (a BGZF block always fits)
    // lines for the host (cto_pon_host_lines)
    std::string hl_bytes;
    std::vector<int64_t> hl_off{0}, hl_line;
};

namespace {

// one scan of one file (or one tabix chunk after another): the slab loop's state
struct Scan {
    cto_pon* c;
    hipStream_t s;
    int cr;                      // '\r' ends a line too (gzip -dc through TextIOWrapper(newline=''))
    int only;                    // k_pon_parse's `only`
    int only_len;
    int require_allele;
    cto_pon_stats* st;
    int cur = 0;                 // text buffer the next slab is written to
    size_t carry = 0;            // bytes of an unfinished line at its front
    int64_t line_base = 0;       // lines of the file before the slab

    uint8_t* text() const { return c->text[cur].as<uint8_t>(); }
    // room for `n` more bytes behind the carried ones in the current text buffer (its carry survives growth)
    int reserve(size_t n) {
        DevBuf& t = c->text[cur];
        if (carry + n + 16 <= t.cap) return CTO_OK;
        DevBuf& o = c->text[cur ^ 1];
        if (o.ensure(carry + n + 16) != CTO_OK) return CTO_EHIP;
        if (carry) CTO_HIP(hipMemcpyAsync(o.p, t.p, carry, hipMemcpyDeviceToDevice, s));
        cur ^= 1;
        return CTO_OK;
    }

    // the slab text[0, carry + n): line starts, the parse of every finished line, the unfinished one carried
    int lines(size_t n, bool eof) {
        const size_t T = carry + n;
        if (T == 0) return CTO_OK;
        CTO_REQUIRE(T < (size_t(1) << 32) - LINE_TILE, CTO_EINVAL, "cto_pon_match_file: a line of more than 4 GB");
        const uint32_t n32 = uint32_t(T);
        const int tiles = int(cdiv(int64_t(T), LINE_TILE));
        if (c->tiles.ensure(sizeof(int) * size_t(tiles)) || c->tile_base.ensure(sizeof(int) * size_t(tiles + 1)) ||
            c->tile_tmp.ensure(sizeof(long long) * size_t(cdiv(tiles, SCAN_TILE) + 1)) || c->tile_tot.ensure(sizeof(long long)) ||
            c->counters.ensure(2 * sizeof(unsigned)) || c->h_small.ensure(64))
            return CTO_EHIP;
        hipLaunchKernelGGL(k_line_count, dim3(unsigned(tiles)), dim3(1024), 0, s, text(), n32, cr, c->tiles.as<int>());
        scan_exclusive<int>(s, c->tiles.as<int>(), tiles, c->tile_base.as<int>(), nullptr, c->tile_tmp.as<long long>(), c->tile_tot.as<long long>());
        CTO_HIP(hipGetLastError());
        uint8_t* hs = c->h_small.as<uint8_t>();
        CTO_HIP(hipMemcpyAsync(hs, c->tile_base.as<int>() + tiles, sizeof(int), hipMemcpyDeviceToHost, s));
        CTO_HIP(hipMemcpyAsync(hs + 4, text() + T - 1, 1, hipMemcpyDeviceToHost, s));
        CTO_HIP(record_and_wait(c->ev, s));
        int n_lines = 0;
        memcpy(&n_lines, hs, 4);
        const uint8_t last = hs[4];
        if (c->starts.ensure(sizeof(uint32_t) * size_t(n_lines + 1)) || c->host_idx.ensure(sizeof(uint32_t) * size_t(n_lines + 1))) return CTO_EHIP;
        hipLaunchKernelGGL(k_line_emit, dim3(unsigned(tiles)), dim3(1024), 0, s, text(), n32, cr, c->tile_base.as<int>(), c->starts.as<uint32_t>());
        const bool whole = eof || last == '\n';      // a slab ending in '\r' carries that line: "\r\n" may be cut between slabs
        const uint32_t n_proc = uint32_t(whole ? n_lines : n_lines - 1);
        CTO_HIP(hipMemsetAsync(c->counters.p, 0, 2 * sizeof(unsigned), s));
        if (n_proc > 0) {
            DevCalls cs{c->pos.as<int64_t>(), c->ctg_off.as<int64_t>(), c->orig.as<int64_t>(), c->str_off.as<int64_t>(), c->str.as<uint8_t>(),
                        c->name_off.as<int64_t>(), c->name_bytes.as<uint8_t>(), c->n_ctg};
            hipLaunchKernelGGL(k_pon_parse, dim3(unsigned(cdiv(n_proc, 256))), dim3(256), 0, s, text(), n32, c->starts.as<uint32_t>(), uint32_t(n_lines),
                               n_proc, cs, only, c->only_name.as<uint8_t>(), only_len, require_allele, c->hit.as<uint8_t>(), c->host_idx.as<uint32_t>(),
                               c->counters.as<unsigned>());
        }
        CTO_HIP(hipGetLastError());
        CTO_HIP(hipMemcpyAsync(hs + 8, c->counters.p, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, s));
        uint32_t carry_from = n32;
        if (!whole) CTO_HIP(hipMemcpyAsync(hs + 16, c->starts.as<uint32_t>() + n_lines - 1, 4, hipMemcpyDeviceToHost, s));
        CTO_HIP(record_and_wait(c->ev, s));
        unsigned cnt[2];
        memcpy(cnt, hs + 8, 8);
        if (!whole) memcpy(&carry_from, hs + 16, 4);
        st->records += cnt[1];
        st->host_lines += cnt[0];
        if (cnt[0]) {                                         // rare: fetch those lines, in file order
            std::vector<uint32_t> idx(cnt[0]), sv(size_t(n_lines) + 1);
            CTO_HIP(hipMemcpy(idx.data(), c->host_idx.p, sizeof(uint32_t) * cnt[0], hipMemcpyDeviceToHost));
            CTO_HIP(hipMemcpy(sv.data(), c->starts.p, sizeof(uint32_t) * size_t(n_lines), hipMemcpyDeviceToHost));
            sv[size_t(n_lines)] = n32;
            std::sort(idx.begin(), idx.end());
            for (uint32_t k : idx) {
                const size_t a = sv[k], b = k + 1 < uint32_t(n_lines) ? sv[k + 1] : n32;
                const size_t at = c->hl_bytes.size();
                c->hl_bytes.resize(at + (b - a));
                CTO_HIP(hipMemcpy(&c->hl_bytes[at], text() + a, b - a, hipMemcpyDeviceToHost));
                c->hl_off.push_back(int64_t(c->hl_bytes.size()));
                c->hl_line.push_back(line_base + k + 1);
            }
        }
        line_base += n_proc;
        const size_t keep = T - carry_from;
        if (keep) {                                           // the unfinished line goes to the front of the other buffer
            if (c->text[cur ^ 1].ensure(keep + c->text_cap + 16)) return CTO_EHIP;
            CTO_HIP(hipMemcpyAsync(c->text[cur ^ 1].p, text() + carry_from, keep, hipMemcpyDeviceToDevice, s));
            cur ^= 1;
        }
        carry = keep;
        return CTO_OK;
    }

    // text already in host memory (plain .vcf slabs, host-inflated gzip): up, then lines()
    int host_text(const uint8_t* p, size_t n, bool eof) {
        if (reserve(n)) return CTO_EHIP;
        if (n) CTO_HIP(hipMemcpyAsync(text() + carry, p, n, hipMemcpyHostToDevice, s));
        return lines(n, eof);
    }
};

// BGZF blocks of file bytes [beg, end) inflated on the device (end: the file offset of the first block not to read; a block at `tail_block`
// contributes only its first tail_keep bytes, the first block only from head_skip on).  Returns 1 when the bytes are not BGZF throughout
// (the caller reads the file as other gzip), CTO_OK, or an error.
int bgzf_range(Scan& sc, FILE* f, int64_t beg, int64_t end, uint32_t head_skip, int64_t tail_block, uint32_t tail_keep, bool last_range) {
    cto_pon* c = sc.c;
    hipStream_t s = sc.s;
    if (c->h_in.ensure(c->slab_in + CTO_BGZF_PAD) || c->comp.ensure(c->slab_in + CTO_BGZF_PAD) || c->status.ensure(sizeof(int) * (c->slab_in / 18 + 1)))
        return CTO_EHIP;
    c->h_blocks.resize(c->slab_in / 18 + 1);
    const int64_t read_end = tail_block >= 0 ? tail_block + 65536 + 64 : end;    // a BGZF block is at most 64 KiB
    int64_t fpos = beg;                       // file offset of h_in[0]
    size_t have = 0;
    bool at_eof = false;
    CTO_REQUIRE(fseeko(f, beg, SEEK_SET) == 0, CTO_EINVAL, "cto_pon_match_file: cannot seek");
    for (;;) {
        uint8_t* in = c->h_in.as<uint8_t>();
        if (!at_eof) {
            const size_t want = size_t(std::min<int64_t>(int64_t(c->slab_in) - int64_t(have), read_end - (fpos + int64_t(have))));
            const size_t got = want ? fread(in + have, 1, want, f) : 0;
            sc.st->bytes_read += int64_t(got);
            have += got;
            if (got < want || fpos + int64_t(have) >= read_end) at_eof = true;
        }
        int64_t out_bytes = 0;
        int64_t nb = cto_bgzf_scan(in, have, fpos, c->h_blocks.data(), int64_t(c->h_blocks.size()), &out_bytes);
        if (nb < 0) return 1;
        // the slab: whole blocks inside the range, up to c->text_cap inflated bytes
        int64_t take = 0, text_n = 0;
        c->h_pieces.clear();
        bool range_done = false;
        for (; take < nb; ++take) {
            const cto_bgzf_block& b = c->h_blocks[size_t(take)];
            const int64_t off = int64_t(b.file_off);
            const bool is_tail = off == tail_block;
            if (off >= end && !is_tail) { range_done = true; break; }
            if (take > 0 && text_n + int64_t(b.isize) > int64_t(c->text_cap)) break;
            const int64_t from = off == beg ? std::min<int64_t>(head_skip, b.isize) : 0;
            const int64_t to = is_tail ? std::min<int64_t>(tail_keep, b.isize) : int64_t(b.isize);
            if (to > from) {
                c->h_pieces.push_back(int64_t(b.out_off) + from);
                c->h_pieces.push_back(to - from);
                c->h_pieces.push_back(int64_t(sc.carry) + text_n);
                text_n += to - from;
            }
            if (is_tail) { range_done = true; ++take; break; }
        }
        const size_t used = take > 0 ? size_t(c->h_blocks[size_t(take - 1)].file_off + c->h_blocks[size_t(take - 1)].bsize - uint64_t(fpos)) : 0;
        if (take == nb && at_eof && used < have && !range_done) return 1;    // a cut or foreign member at the end of the file
        if (take > 0) {
            const int64_t slot_bytes = int64_t(c->h_blocks[size_t(take - 1)].out_off) + (int64_t(c->h_blocks[size_t(take - 1)].isize) + CTO_BGZF_SLOT_PAD + 255) / 256 * 256;
            if (c->slots.ensure(size_t(slot_bytes) + 256) || c->blocks.ensure(sizeof(cto_bgzf_block) * size_t(take)) ||
                c->pieces.ensure(sizeof(int64_t) * (c->h_pieces.size() + 3)) || sc.reserve(size_t(text_n)))
                return CTO_EHIP;
            CTO_HIP(hipMemcpyAsync(c->comp.p, in, used, hipMemcpyHostToDevice, s));   // the kernel's over-read stays inside comp's CTO_BGZF_PAD
            CTO_HIP(hipMemcpyAsync(c->blocks.p, c->h_blocks.data(), sizeof(cto_bgzf_block) * size_t(take), hipMemcpyHostToDevice, s));
            CTO_HIP(hipMemcpyAsync(c->pieces.p, c->h_pieces.data(), sizeof(int64_t) * c->h_pieces.size(), hipMemcpyHostToDevice, s));
            int rc = cto_bgzf_inflate(c->comp.p, c->blocks.as<cto_bgzf_block>(), int(take), c->slots.p, c->status.as<int>(), s);
            if (rc) return rc;
            std::vector<int> bstat(static_cast<size_t>(take));
            CTO_HIP(hipMemcpyAsync(bstat.data(), c->status.p, sizeof(int) * size_t(take), hipMemcpyDeviceToHost, s));
            const unsigned n_pieces = unsigned(c->h_pieces.size() / 3);
            if (n_pieces) hipLaunchKernelGGL(k_gather, dim3(n_pieces), dim3(256), 0, s, c->slots.as<uint8_t>(), c->pieces.as<int64_t>(), sc.text());
            CTO_HIP(hipGetLastError());
            CTO_HIP(record_and_wait(c->ev, s));
            for (int x : bstat)
                if (x != 0) return 1;                                  // a block zlib would read differently: the host path decides
            sc.st->blocks_device += take;
            sc.st->bytes_inflated += text_n;
        }
        memmove(in, in + used, have - used);
        fpos += int64_t(used);
        have -= used;
        const bool done = range_done || (at_eof && take == nb);
        if (int rc = sc.lines(size_t(text_n), done && last_range)) return rc;
        if (done) return CTO_OK;
        CTO_REQUIRE(take > 0, CTO_EINVAL, "cto_pon_match_file: BGZF block larger than the slab");
    }
}

}  // namespace

extern "C" int cto_pon_create(cto_pon** out) try {
    CTO_REQUIRE(out, CTO_EINVAL, "cto_pon_create: null argument");
    std::unique_ptr<cto_pon> c(new cto_pon());
    if (const int rc = c->ev.create(hipEventDisableTiming)) return rc;
    *out = c.release();
    return CTO_OK;
}
CTO_CATCH("cto_pon_create", int)

extern "C" void cto_pon_destroy(cto_pon* c) { delete c; }

extern "C" int cto_pon_set_calls(cto_pon* c, int n_ctg, const char* ctg_bytes, const int64_t* ctg_off, int64_t n_calls, const int32_t* call_ctg,
                                 const int64_t* call_pos, const char* str_bytes, const int64_t* str_off) try {
    CTO_REQUIRE(c && n_ctg >= 0 && n_calls >= 0 && (n_ctg == 0 || (ctg_bytes && ctg_off)) &&
                (n_calls == 0 || (call_ctg && call_pos && str_bytes && str_off)), CTO_EINVAL, "cto_pon_set_calls: null argument");
    std::vector<int64_t> order(static_cast<size_t>(n_calls));
    for (int64_t i = 0; i < n_calls; ++i) {
        CTO_REQUIRE(call_ctg[i] >= 0 && call_ctg[i] < n_ctg, CTO_EINVAL, "cto_pon_set_calls: call %lld names contig %d", (long long)i, call_ctg[i]);
        order[size_t(i)] = i;
    }
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
        return call_ctg[a] != call_ctg[b] ? call_ctg[a] < call_ctg[b] : call_pos[a] < call_pos[b]; });
    std::vector<int64_t> pos(static_cast<size_t>(n_calls)), coff(size_t(n_ctg) + 1, 0), soff(size_t(2 * n_calls) + 1, 0);
    std::string str;
    for (int64_t j = 0; j < n_calls; ++j) {
        const int64_t i = order[size_t(j)];
        pos[size_t(j)] = call_pos[i];
        ++coff[size_t(call_ctg[i]) + 1];
        for (int h = 0; h < 2; ++h) {
            str.append(str_bytes + str_off[2 * i + h], size_t(str_off[2 * i + h + 1] - str_off[2 * i + h]));
            soff[size_t(2 * j + h + 1)] = int64_t(str.size());
        }
    }
    for (int k = 0; k < n_ctg; ++k) coff[size_t(k) + 1] += coff[size_t(k)];
    c->names.clear();
    for (int k = 0; k < n_ctg; ++k) c->names.emplace_back(ctg_bytes + ctg_off[k], size_t(ctg_off[k + 1] - ctg_off[k]));
    auto up = [&](DevBuf& d, const void* h, size_t n) -> int {
        if (d.ensure(n + 16)) return CTO_EHIP;
        if (n) CTO_HIP(hipMemcpy(d.p, h, n, hipMemcpyHostToDevice));
        return CTO_OK;
    };
    std::vector<int64_t> noff(size_t(n_ctg) + 1);
    for (int k = 0; k <= n_ctg; ++k) noff[size_t(k)] = ctg_off[k] - ctg_off[0];
    if (up(c->pos, pos.data(), 8 * pos.size()) || up(c->ctg_off, coff.data(), 8 * coff.size()) || up(c->orig, order.data(), 8 * order.size()) ||
        up(c->str_off, soff.data(), 8 * soff.size()) || up(c->str, str.data(), str.size()) || up(c->name_off, noff.data(), 8 * noff.size()) ||
        up(c->name_bytes, n_ctg ? ctg_bytes + ctg_off[0] : nullptr, size_t(noff.back())) || c->hit.ensure(size_t(n_calls) + 16))
        return CTO_EHIP;
    c->n_ctg = n_ctg;
    c->n_calls = n_calls;
    return CTO_OK;
}
CTO_CATCH("cto_pon_set_calls", int)

namespace {
// what `gzip -dc` prints, inflated on the host slab by slab and scanned on the device: gzip members one after another; bytes after a
// member that do not start another one are ignored; a damaged or cut member ends the text where zlib stops
int host_gzip(Scan& sc, FILE* f) {
    cto_pon* c = sc.c;
    std::vector<uint8_t> in(size_t(1) << 22);
    const uint8_t* next = in.data();
    size_t avail = 0;
    bool file_eof = false;
    auto want = [&](size_t n) {                  // at least n bytes of input in view, unless the file ends first
        if (avail >= n || file_eof) return;
        memmove(in.data(), next, avail);
        const size_t got = fread(in.data() + avail, 1, in.size() - avail, f);
        sc.st->bytes_read += int64_t(got);
        file_eof = got < in.size() - avail;
        next = in.data();
        avail += got;
    };
    z_stream z{};
    if (inflateInit2(&z, 16 + MAX_WBITS) != Z_OK) { set_error("cto_pon_match_file: zlib"); return CTO_ENOMEM; }
    std::unique_ptr<z_stream, int (*)(z_stream*)> zguard(&z, inflateEnd);
    uint8_t* out = c->h_in.as<uint8_t>();
    size_t have = 0;
    bool member = false;
    for (;;) {
        if (!member) {
            want(2);
            if (!is_gzip_magic(next, avail)) break;
            inflateReset(&z);
            member = true;
        }
        want(1);
        z.next_in = const_cast<Bytef*>(next);
        z.avail_in = uInt(avail);
        z.next_out = out + have;
        z.avail_out = uInt(c->slab_in - have);
        const int rc = inflate(&z, Z_NO_FLUSH);
        const size_t used = avail - z.avail_in, made = (c->slab_in - have) - z.avail_out;
        next += used;
        avail -= used;
        have += made;
        sc.st->bytes_inflated += int64_t(made);
        if (rc == Z_STREAM_END) member = false;
        else if (rc != Z_OK && !(rc == Z_BUF_ERROR && (used || made))) break;
        if (have == c->slab_in) {
            if (int e = sc.host_text(out, have, false)) return e;
            have = 0;
        }
    }
    return sc.host_text(out, have, true);
}

// the inflated .tbi at `path` -> the contig's chunks; false when the index cannot be read or parsed
bool tbi_chunks(const char* path, size_t size, const char* ctg, std::vector<Chunk>* chunks, bool* found) {
    std::vector<uint8_t> raw(size), idx;
    FILE* g = fopen(path, "rb");
    if (!g) return false;
    const bool ok = fread(raw.data(), 1, raw.size(), g) == raw.size();
    fclose(g);
    std::string err;
    return ok && gunzip_mem(raw.data(), raw.size(), &idx) && tbi_contig_chunks(idx.data(), idx.size(), ctg, chunks, found, &err);
}

// the index or the BGZF path gave up half way: nothing it found counts
int restart(cto_pon* c, Scan& sc, cto_pon_stats* st, hipStream_t s) {
    CTO_HIP(hipMemsetAsync(c->hit.p, 0, size_t(c->n_calls), s));
    c->hl_bytes.clear();
    c->hl_off.assign(1, 0);
    c->hl_line.clear();
    *st = cto_pon_stats{};
    sc = Scan{c, s, 1, sc.only, sc.only_len, sc.require_allele, st};
    return CTO_OK;
}

int match_file(cto_pon* c, const char* path, const char* only_contig, int require_allele, cto_pon_stats* st, hipStream_t s) {
    FILE* f = fopen(path, "rb");
    CTO_REQUIRE(f, CTO_EINVAL, "cto_pon_match_file: cannot open %s", path);
    std::unique_ptr<FILE, int (*)(FILE*)> guard(f, fclose);
    const std::string p(path);
    const bool plain = p.size() >= 4 && p.compare(p.size() - 4, 4, ".vcf") == 0;
    Scan sc{c, s, plain ? 0 : 1, -2, 0, require_allele, st};
    if (only_contig) {
        const int n = int(strlen(only_contig));
        if (c->only_name.ensure(size_t(n) + 16)) return CTO_EHIP;
        if (n) CTO_HIP(hipMemcpy(c->only_name.p, only_contig, size_t(n), hipMemcpyHostToDevice));
        sc.only = -1;
        sc.only_len = n;
        for (int k = 0; k < c->n_ctg; ++k)
            if (c->names[size_t(k)] == only_contig) sc.only = k;
    }
    if (c->h_in.ensure(c->slab_in + CTO_BGZF_PAD)) return CTO_EHIP;
    if (plain) {
        st->kind = 0;
        for (;;) {
            const size_t got = fread(c->h_in.p, 1, c->slab_in, f);
            st->bytes_read += int64_t(got);
            st->bytes_inflated += int64_t(got);
            const bool eof = got < c->slab_in;
            if (int rc = sc.host_text(c->h_in.as<uint8_t>(), got, eof)) return rc;
            if (eof) return CTO_OK;
        }
    }
    uint8_t head[32] = {0};
    const size_t nh = fread(head, 1, sizeof head, f);
    st->bytes_read += int64_t(nh);
    if (!is_gzip_magic(head, nh)) { st->kind = 3; return CTO_OK; }          // gzip -dc prints nothing
    if (is_bgzf_header(head, nh)) {
        struct stat sb;
        CTO_REQUIRE(fstat(fileno(f), &sb) == 0, CTO_EINVAL, "cto_pon_match_file: cannot stat %s", path);
        const std::string tbi = p + ".tbi";
        struct stat tb;
        if (only_contig && c->n_calls > 0 && p.size() >= 3 && p.compare(p.size() - 3, 3, ".gz") == 0 && stat(tbi.c_str(), &tb) == 0) {
            // the contig's chunks only; an index that cannot be read, does not parse or names bytes that are not BGZF is not used: the
            // whole file is scanned instead (the reference falls back the same way when tabix fails, and reads no index without tabix)
            std::vector<Chunk> chunks;
            bool found = false;
            if (tbi_chunks(tbi.c_str(), size_t(tb.st_size), only_contig, &chunks, &found)) {
                st->kind = 1;
                st->used_tbi = 1;
                int rc = 0;
                for (size_t i = 0; i < chunks.size() && rc == 0; ++i) {
                    const int64_t cb = int64_t(chunks[i].beg >> 16), ce = int64_t(chunks[i].end >> 16);
                    const uint32_t ue = uint32_t(chunks[i].end & 0xffff);
                    sc.carry = 0;
                    rc = bgzf_range(sc, f, cb, ce, uint32_t(chunks[i].beg & 0xffff), ue ? ce : -1, ue, true);
                }
                if (rc != 1) return rc;
                if (int e = restart(c, sc, st, s)) return e;
            }
        }
        st->kind = 1;
        const int rc = bgzf_range(sc, f, 0, int64_t(sb.st_size), 0, -1, 0, true);
        if (rc != 1) return rc;
        if (int e = restart(c, sc, st, s)) return e;                 // not BGZF throughout: start again on the host path
    }
    st->kind = 2;
    CTO_REQUIRE(fseeko(f, 0, SEEK_SET) == 0, CTO_EINVAL, "cto_pon_match_file: cannot seek %s", path);
    return host_gzip(sc, f);
}
}  // namespace

extern "C" int cto_pon_match_file(cto_pon* c, const char* path, const char* only_contig, int require_allele, uint8_t* hit, cto_pon_stats* stats,
                                  void* stream) try {
    CTO_REQUIRE(c && path && (hit || c->n_calls == 0) && stats, CTO_EINVAL, "cto_pon_match_file: null argument");
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t s = static_cast<hipStream_t>(stream);
    *stats = cto_pon_stats{};
    const char* env = getenv("CTO_PON_SLAB");
    c->slab_in = env && atoll(env) >= (1 << 17) ? size_t(atoll(env)) : SLAB_DEFAULT;
    c->text_cap = 4 * c->slab_in;
    c->hl_bytes.clear();
    c->hl_off.assign(1, 0);
    c->hl_line.clear();
    if (c->hit.ensure(size_t(c->n_calls) + 16)) return CTO_EHIP;
    CTO_HIP(hipMemsetAsync(c->hit.p, 0, size_t(c->n_calls) + 16, s));
    if (int rc = match_file(c, path, only_contig, require_allele, stats, s)) return rc;
    if (c->n_calls) CTO_HIP(hipMemcpyAsync(hit, c->hit.p, size_t(c->n_calls), hipMemcpyDeviceToHost, s));
    CTO_HIP(record_and_wait(c->ev, s));
    stats->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return CTO_OK;
}
CTO_CATCH("cto_pon_match_file", int)

extern "C" int64_t cto_pon_host_lines(cto_pon* c, const char** bytes, const int64_t** off, const int64_t** line_no) {
    if (!c || !bytes || !off || !line_no) { set_error("cto_pon_host_lines: null argument"); return CTO_EINVAL; }
    *bytes = c->hl_bytes.data();
    *off = c->hl_off.data();
    *line_no = c->hl_line.data();
    return int64_t(c->hl_line.size());
}

extern "C" int64_t cto_tbi_contig_chunks(const uint8_t* tbi_file, size_t len, const char* ctg, uint64_t* chunks, int64_t cap) try {
    CTO_REQUIRE(tbi_file && ctg && (chunks || cap == 0), CTO_EINVAL, "cto_tbi_contig_chunks: null argument");
    std::vector<uint8_t> idx;
    std::vector<Chunk> out;
    bool found = false;
    std::string err;
    CTO_REQUIRE(gunzip_mem(tbi_file, len, &idx), CTO_EINVAL, "cto_tbi_contig_chunks: not gzip");
    CTO_REQUIRE(tbi_contig_chunks(idx.data(), idx.size(), ctg, &out, &found, &err), CTO_EINVAL, "cto_tbi_contig_chunks: %s", err.c_str());
    CTO_REQUIRE(int64_t(out.size()) <= cap, CTO_ENOMEM, "cto_tbi_contig_chunks: %zu chunks", out.size());
    for (size_t i = 0; i < out.size(); ++i) {
        chunks[2 * i] = out[i].beg;
        chunks[2 * i + 1] = out[i].end;
    }
    return int64_t(out.size());
}
CTO_CATCH("cto_tbi_contig_chunks", int64_t)
