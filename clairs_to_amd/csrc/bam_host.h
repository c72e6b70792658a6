// The host's reader of BGZF, the binning indices (BAI, TBI) and BAM alignment records - the one statement of each that the host
// consumers are written on (csrc/bam.cpp: the pile-up producer, the allele counter's host rules, the SAM text writer; csrc/pon.hip:
// the tabix query).  Standard library, zlib, dl and the C header only, so that a plain C++ compiler - and a sanitizer - sees it
// (tests/host/bam_host_check.cpp).  The device states the same record grammar on its own (bam_records.h), and the tests hold the two
// equal: nothing here is shared with it.
#pragma once
#include <dlfcn.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <climits>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/clairsto_amd.h"

namespace cto {

inline int32_t le32(const uint8_t* p) { return int32_t(uint32_t(p[0]) | (uint32_t(p[1]) << 8) | (uint32_t(p[2]) << 16) | (uint32_t(p[3]) << 24)); }
inline uint64_t le64(const uint8_t* p) { return uint64_t(uint32_t(le32(p))) | (uint64_t(uint32_t(le32(p + 4))) << 32); }

// ------------------------------------------------------------------------------------------------ BGZF
// libdeflate inflates BGZF blocks 2-3x faster than zlib.  Its headers are not installed here, only the runtime library, so
// the three entry points of its stable v1 ABI are resolved with dlopen; zlib remains the fallback.
struct LibDeflate {
    void* h = nullptr;
    void* (*alloc)() = nullptr;
    int (*inflate)(void*, const void*, size_t, void*, size_t, size_t*) = nullptr;
    uint32_t (*crc)(uint32_t, const void*, size_t) = nullptr;
    void (*release)(void*) = nullptr;
    LibDeflate() {
        if (getenv("CTO_NO_LIBDEFLATE")) return;
        for (const char* name : {"libdeflate.so.0", "libdeflate.so"}) {
            h = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (h) break;
        }
        if (!h) return;
        alloc = reinterpret_cast<void* (*)()>(dlsym(h, "libdeflate_alloc_decompressor"));
        inflate = reinterpret_cast<int (*)(void*, const void*, size_t, void*, size_t, size_t*)>(dlsym(h, "libdeflate_deflate_decompress"));
        release = reinterpret_cast<void (*)(void*)>(dlsym(h, "libdeflate_free_decompressor"));
        crc = reinterpret_cast<uint32_t (*)(uint32_t, const void*, size_t)>(dlsym(h, "libdeflate_crc32"));
        if (!alloc || !inflate || !release) { alloc = nullptr; inflate = nullptr; release = nullptr; }
    }
    bool ok() const { return inflate != nullptr; }
};
inline const LibDeflate& libdeflate() {
    static const LibDeflate ld;
    return ld;
}

// CRC-32 of a BGZF block's inflated bytes (the gzip trailer holds the expected value; htslib checks it too)
inline uint32_t block_crc(const uint8_t* p, size_t n) {
    if (libdeflate().crc) return libdeflate().crc(0, p, n);
    return uint32_t(crc32(crc32(0L, Z_NULL, 0), p, uInt(n)));
}

// The header of the BGZF block at h[0 .. avail) (SAM specification, section 4.1): the BC subfield is normally first, the extra field
// is scanned in general.  MORE = the block does not lie inside the bytes given; xlen is valid from 18 bytes on, bsize (0 until the BC
// subfield is seen) as far as the bytes reach.  What MORE means - a damaged file, a range that ends inside a block - is the caller's.
struct BgzfHeader {
    enum Status { OK, NOT_BGZF, NO_BC, BAD_SIZE, TOO_LARGE, MORE };
    int xlen = 0, bsize = 0, cdata = 0;     // extra field; whole block; deflate payload (at h + 12 + xlen; CRC32 and ISIZE follow it)
    uint32_t isize = 0, crc32 = 0;
};
inline BgzfHeader::Status bgzf_header(const uint8_t* h, size_t avail, BgzfHeader* out) {
    *out = BgzfHeader{};
    if (avail < 18) return BgzfHeader::MORE;
    if (h[0] != 31 || h[1] != 139 || h[2] != 8 || !(h[3] & 4)) return BgzfHeader::NOT_BGZF;
    const size_t xlen = size_t(h[10]) | (size_t(h[11]) << 8);
    out->xlen = int(xlen);
    for (size_t i = 0; i + 4 <= xlen && 12 + i + 4 <= avail;) {
        const uint8_t* e = h + 12 + i;
        const size_t slen = size_t(e[2]) | (size_t(e[3]) << 8);
        if (e[0] == 'B' && e[1] == 'C' && slen == 2 && i + 6 <= xlen && 12 + i + 6 <= avail) out->bsize = (e[4] | (e[5] << 8)) + 1;
        i += 4 + slen;
    }
    if (avail < 12 + xlen) return BgzfHeader::MORE;
    if (out->bsize == 0) return BgzfHeader::NO_BC;
    out->cdata = out->bsize - int(xlen) - 12 - 8;
    if (out->cdata < 0) return BgzfHeader::BAD_SIZE;
    if (avail < size_t(out->bsize)) return BgzfHeader::MORE;
    const uint8_t* tail = h + out->bsize - 8;
    out->crc32 = uint32_t(le32(tail));
    out->isize = uint32_t(le32(tail + 4));
    return out->isize > 65536 ? BgzfHeader::TOO_LARGE : BgzfHeader::OK;     // the format's limit
}
inline const char* bgzf_why(BgzfHeader::Status st) {     // what is wrong with the header, for every status but OK and MORE
    return st == BgzfHeader::NOT_BGZF ? "not a BGZF block header" : st == BgzfHeader::NO_BC ? "BGZF block without BC subfield"
         : st == BgzfHeader::BAD_SIZE ? "bad BGZF block size" : "BGZF block claims more than 64 KiB of data";
}

// BGZF blocks that were inflated elsewhere (on the device: cto_bgzf_inflate), looked up by their file offset
struct PreInflated {
    const uint8_t* data = nullptr;
    const cto_bgzf_block* blocks = nullptr;     // sorted by file_off
    int64_t n = 0;
    const cto_bgzf_block* find(int64_t coff) const {
        int64_t lo = 0, hi = n;
        while (lo < hi) {
            const int64_t mid = (lo + hi) / 2;
            if (int64_t(blocks[mid].file_off) < coff) lo = mid + 1; else hi = mid;
        }
        return (lo < n && int64_t(blocks[lo].file_off) == coff) ? blocks + lo : nullptr;
    }
};

struct Bgzf {
    const uint8_t* map = nullptr;       // the BAM file, mapped: blocks are inflated straight out of the page cache
    int64_t fsize = 0;
    std::vector<uint8_t> block;         // inflated current block (when it was inflated here)
    const uint8_t* bptr = nullptr;      // the current block's inflated bytes: block.data() or a slot of `pre`
    size_t blen = 0;
    PreInflated pre;
    int64_t block_coffset = -1;         // file offset of the current block
    int64_t next_coffset = 0;           // file offset of the block after it
    size_t upos = 0;                    // read position inside `block`
    z_stream zs;
    bool zs_init = false;
    void* ld = nullptr;                 // libdeflate decompressor when available
    std::string err;

    ~Bgzf() {
        if (zs_init) inflateEnd(&zs);
        if (ld) libdeflate().release(ld);
        if (map && fsize > 0) munmap(const_cast<uint8_t*>(map), size_t(fsize));
    }
    bool open(const char* path) {
        const int fd = ::open(path, O_RDONLY | O_CLOEXEC);
        if (fd < 0) { err = std::string("cannot open ") + path; return false; }
        struct stat st;
        if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) { ::close(fd); err = std::string(path) + " is not a regular file"; return false; }
        fsize = int64_t(st.st_size);
        if (fsize > 0) {
            void* m = mmap(nullptr, size_t(fsize), PROT_READ, MAP_PRIVATE, fd, 0);
            if (m == MAP_FAILED) { ::close(fd); fsize = 0; err = std::string("cannot map ") + path; return false; }
            map = static_cast<const uint8_t*>(m);
        }
        ::close(fd);
        memset(&zs, 0, sizeof(zs));
        if (inflateInit2(&zs, -15) != Z_OK) { err = "inflateInit2 failed"; return false; }
        zs_init = true;
        if (libdeflate().ok()) ld = libdeflate().alloc();
        return true;
    }
    // loads the block that starts at file offset `coff`; false at EOF (err stays empty) or on error
    bool load(int64_t coff) {
        if (const cto_bgzf_block* pb = pre.find(coff)) {        // already inflated: a view, no file access
            bptr = pre.data + pb->out_off;
            blen = pb->isize;
            if (blen && block_crc(bptr, blen) != pb->crc32) { err = "BGZF block fails its CRC-32"; return false; }
            block_coffset = coff;
            next_coffset = coff + int64_t(pb->bsize);
            upos = 0;
            return true;
        }
        if (coff < 0 || coff > fsize) { err = "seek failed"; return false; }
        if (coff == fsize) return false;   // clean EOF
        const uint8_t* h = map + coff;
        const int64_t left = fsize - coff;
        BgzfHeader bh;
        const BgzfHeader::Status st = bgzf_header(h, size_t(left), &bh);
        if (st == BgzfHeader::MORE) {           // the file ends inside the block
            err = left < 18 ? "not a BGZF block header" : (left < 12 + bh.xlen ? "truncated BGZF extra field" : "truncated BGZF block");
            return false;
        }
        if (st != BgzfHeader::OK) { err = bgzf_why(st); return false; }
        const uint8_t* payload = h + 12 + bh.xlen;
        const uint32_t isize = bh.isize;
        block.resize(isize);
        if (isize && ld) {
            size_t got_out = 0;
            if (libdeflate().inflate(ld, payload, size_t(bh.cdata), block.data(), isize, &got_out) != 0 || got_out != isize) {
                err = "inflate failed";
                return false;
            }
        } else if (isize) {
            inflateReset(&zs);
            zs.next_in = const_cast<uint8_t*>(payload);
            zs.avail_in = uInt(bh.cdata);
            zs.next_out = block.data();
            zs.avail_out = uInt(isize);
            const int rc = inflate(&zs, Z_FINISH);
            if (rc != Z_STREAM_END || zs.avail_out != 0) { err = "inflate failed"; return false; }
        }
        if (isize && block_crc(block.data(), isize) != bh.crc32) { err = "BGZF block fails its CRC-32"; return false; }
        bptr = block.data();
        blen = block.size();
        block_coffset = coff;
        next_coffset = coff + bh.bsize;
        upos = 0;
        return true;
    }
    bool seek(uint64_t voff) {
        const int64_t coff = int64_t(voff >> 16);
        if (coff != block_coffset && !load(coff)) return false;
        upos = size_t(voff & 0xffff);
        return upos <= blen;
    }
    // virtual offset of the next byte; the end of a block is reported as the start of the next one, as index chunks do
    uint64_t tell() const {
        if (block_coffset >= 0 && upos >= blen) return uint64_t(next_coffset) << 16;
        return (uint64_t(block_coffset) << 16) | uint64_t(upos);
    }
    // tell() once the block that holds the next byte is loaded: the one name of a record's place that does not depend on how the
    // reader came there (the device derives the same from its block table); at the end of the file, or where the next block does
    // not load, it is tell() and read() reports what is wrong
    uint64_t settle() {
        while (block_coffset >= 0 && upos >= blen && load(next_coffset)) {}
        return tell();
    }
    // reads exactly n bytes across block boundaries; false at EOF / error
    bool read(void* dst, size_t n) {
        uint8_t* d = static_cast<uint8_t*>(dst);
        while (n > 0) {
            if (block_coffset < 0 || upos >= blen) {
                if (!load(block_coffset < 0 ? 0 : next_coffset)) return false;
                if (blen == 0) continue;              // empty blocks (e.g. the EOF marker) are skipped
            }
            const size_t take = std::min(n, blen - upos);
            memcpy(d, bptr + upos, take);
            upos += take;
            d += take;
            n -= take;
        }
        return true;
    }
};

// ------------------------------------------------------------------------------------------------ BAI, TBI
struct Chunk { uint64_t beg, end; };     // virtual offsets: compressed block offset << 16 | offset in the inflated block

// bins that may hold alignments overlapping [beg, end) (0-based), SAM specification section 5.3
inline void reg2bins(int64_t beg, int64_t end, std::vector<uint32_t>* bins) {
    --end;
    bins->push_back(0);
    for (int k = 1 + int(beg >> 26); k <= 1 + int(end >> 26); ++k) bins->push_back(uint32_t(k));
    for (int k = 9 + int(beg >> 23); k <= 9 + int(end >> 23); ++k) bins->push_back(uint32_t(k));
    for (int k = 73 + int(beg >> 20); k <= 73 + int(end >> 20); ++k) bins->push_back(uint32_t(k));
    for (int k = 585 + int(beg >> 17); k <= 585 + int(end >> 17); ++k) bins->push_back(uint32_t(k));
    for (int k = 4681 + int(beg >> 14); k <= 4681 + int(end >> 14); ++k) bins->push_back(uint32_t(k));
}

// chunks of reference `tid` that may overlap [beg, end), merged and sorted, from the binning index in buf[0 .. len) (BAI, or the
// inflated TBI) whose per-reference records start at byte `o` after its n_ref references; false on a malformed index
inline bool index_query(const uint8_t* buf, size_t len, size_t o, int n_ref, int tid, int64_t beg, int64_t end, std::vector<Chunk>* out,
                        std::string* err, std::vector<uint64_t>* linear = nullptr) {
    auto need = [&](size_t n) { return n <= len - o; };       // o <= len throughout
    if (tid < 0 || tid >= n_ref) { *err = "reference not in the index"; return false; }
    std::vector<uint32_t> want;
    reg2bins(beg, end, &want);
    std::sort(want.begin(), want.end());
    std::vector<Chunk> chunks;
    uint64_t min_off = 0;
    for (int r = 0; r <= tid; ++r) {
        if (!need(4)) { *err = "truncated BAI"; return false; }
        const int n_bin = le32(buf + o); o += 4;
        if (n_bin < 0) { *err = "malformed BAI"; return false; }
        for (int b = 0; b < n_bin; ++b) {
            if (!need(8)) { *err = "truncated BAI"; return false; }
            const uint32_t bin = uint32_t(le32(buf + o));
            const int n_chunk = le32(buf + o + 4);
            o += 8;
            if (n_chunk < 0) { *err = "malformed BAI"; return false; }
            if (!need(size_t(n_chunk) * 16)) { *err = "truncated BAI"; return false; }
            if (r == tid && bin != 37450 && std::binary_search(want.begin(), want.end(), bin))
                for (int c = 0; c < n_chunk; ++c) chunks.push_back(Chunk{le64(buf + o + size_t(c) * 16), le64(buf + o + size_t(c) * 16 + 8)});
            o += size_t(n_chunk) * 16;
        }
        if (!need(4)) { *err = "truncated BAI"; return false; }
        const int n_intv = le32(buf + o); o += 4;
        if (n_intv < 0) { *err = "malformed BAI"; return false; }
        if (!need(size_t(n_intv) * 8)) { *err = "truncated BAI"; return false; }
        if (r == tid && n_intv > 0) {
            const int64_t w = std::min<int64_t>(beg >> 14, n_intv - 1);
            min_off = le64(buf + o + size_t(w) * 8);
            if (linear) {
                linear->resize(size_t(n_intv));
                for (int i = 0; i < n_intv; ++i) (*linear)[size_t(i)] = le64(buf + o + size_t(i) * 8);
            }
        }
        o += size_t(n_intv) * 8;
    }
    std::sort(chunks.begin(), chunks.end(), [](const Chunk& a, const Chunk& b) { return a.beg < b.beg; });
    for (const Chunk& c : chunks) {
        if (c.end <= min_off) continue;                       // entirely before the first alignment that can overlap
        Chunk d{std::max(c.beg, min_off), c.end};
        if (!out->empty() && d.beg <= out->back().end) out->back().end = std::max(out->back().end, d.end);
        else out->push_back(d);
    }
    return true;
}

inline bool read_index_file(const char* path, std::vector<uint8_t>* buf, std::string* err) {
    FILE* f = fopen(path, "rb");
    if (!f) { *err = std::string("cannot open index ") + path; return false; }
    off_t sz = -1;
    if (fseeko(f, 0, SEEK_END) == 0) sz = ftello(f);
    if (sz < 0 || sz > (off_t(1) << 32) || fseeko(f, 0, SEEK_SET) != 0) {       // not seekable (a pipe, a directory) or absurdly large
        fclose(f);
        *err = std::string("cannot read index ") + path;
        return false;
    }
    buf->resize(size_t(sz));
    const bool ok = fread(buf->data(), 1, buf->size(), f) == buf->size();
    fclose(f);
    if (!ok) { *err = std::string("cannot read index ") + path; return false; }
    return true;
}

inline bool bai_query(const char* path, int tid, int64_t beg, int64_t end, std::vector<Chunk>* out, std::string* err,
                      std::vector<uint64_t>* linear = nullptr) {
    std::vector<uint8_t> buf;
    if (!read_index_file(path, &buf, err)) return false;
    if (buf.size() < 8 || memcmp(buf.data(), "BAI\1", 4) != 0) { *err = "not a BAI index"; return false; }
    return index_query(buf.data(), buf.size(), 8, le32(buf.data() + 4), tid, beg, end, out, err, linear);
}

// The tabix index (SAM/htslib specification, "TBI"): the same binning index as a BAI behind a header that names the sequences.
// `tbi` is the index INFLATED (a .tbi file is BGZF).  The chunks that may hold records of contig `ctg` anywhere on it, merged and
// sorted; *found = false (and no chunks) when the index does not name the contig.
inline bool tbi_contig_chunks(const uint8_t* tbi, size_t len, const char* ctg, std::vector<Chunk>* out, bool* found, std::string* err) {
    *found = false;
    if (len < 36 || memcmp(tbi, "TBI\1", 4) != 0) { *err = "not a tabix index"; return false; }
    const int n_ref = le32(tbi + 4);
    const int l_nm = le32(tbi + 32);
    if (n_ref < 0 || l_nm < 0 || 36 + size_t(l_nm) > len) { *err = "malformed tabix index"; return false; }
    int tid = -1, i = 0;
    for (size_t o = 36; o < 36 + size_t(l_nm) && i < n_ref; ++i) {        // NUL-terminated names, in reference-id order
        const char* nm = reinterpret_cast<const char*>(tbi + o);
        const size_t n = strnlen(nm, 36 + size_t(l_nm) - o);
        if (tid < 0 && strlen(ctg) == n && memcmp(nm, ctg, n) == 0) tid = i;
        o += n + 1;
    }
    if (tid < 0) return true;
    *found = true;
    return index_query(tbi, len, 36 + size_t(l_nm), n_ref, tid, 0, int64_t(1) << 29, out, err);   // the whole contig
}

// ------------------------------------------------------------------------------------------------ alignment records
inline bool consumes_ref(int opc) { return opc == 0 || opc == 2 || opc == 3 || opc == 7 || opc == 8; }       // M D N = X
inline bool consumes_query(int opc) { return opc == 0 || opc == 1 || opc == 4 || opc == 7 || opc == 8; }     // M I S = X

// One auxiliary field (SAM specification, section 4.2.4): A c C take 1 byte, s S 2, i I f 4, Z and H run to their NUL, B is a subtype
// byte, a 32-bit count and count elements of 1 (c C), 2 (s S) or 4 bytes.  val[0 .. len) is the whole value (of a B: from its subtype
// byte on).  aux_next steps over the field at *p; false - the walk ends - when fewer than three bytes are left, the type is unknown
// or the field does not lie wholly in front of `end` (a Z without its NUL, a B whose header or array is cut, a scalar cut short).
struct AuxField {
    char t0, t1, type;
    const uint8_t* val;
    size_t len;
};
inline bool aux_next(const uint8_t** p, const uint8_t* end, AuxField* f) {
    if (end - *p < 3) return false;
    const uint8_t* v = *p + 3;
    const size_t left = size_t(end - v);
    const char ty = char(v[-1]);
    size_t len = 0;
    if (ty == 'A' || ty == 'c' || ty == 'C') len = 1;
    else if (ty == 's' || ty == 'S') len = 2;
    else if (ty == 'i' || ty == 'I' || ty == 'f') len = 4;
    else if (ty == 'Z' || ty == 'H') {
        const void* nul = memchr(v, 0, left);
        if (!nul) return false;
        len = size_t(static_cast<const uint8_t*>(nul) - v) + 1;
    } else if (ty == 'B') {
        if (left < 5) return false;
        const char sub = char(v[0]);
        len = 5 + size_t(uint32_t(le32(v + 1))) * ((sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4);
    } else return false;
    if (len > left) return false;
    *f = AuxField{char(v[-3]), char(v[-2]), ty, v, len};
    *p = v + len;
    return true;
}
// the value of a field of one of the six integer types
inline bool aux_int(const AuxField& f, long long* val) {
    switch (f.type) {
        case 'c': *val = int8_t(f.val[0]); return true;
        case 'C': *val = f.val[0]; return true;
        case 's': *val = int16_t(f.val[0] | (f.val[1] << 8)); return true;
        case 'S': *val = f.val[0] | (f.val[1] << 8); return true;
        case 'i': *val = le32(f.val); return true;
        case 'I': *val = uint32_t(le32(f.val)); return true;
        default: return false;
    }
}

// An alignment record: the fixed fields as BamRegion::next decodes them, and - once BamRegion::lay_out has accepted it - where its
// variable-length fields lie in BamRegion::rec, its operations and what they sum to.
struct BamRecord {
    int pos, l_name, mapq, n_cig, flag, l_seq, next_ref, next_pos, tlen;
    const uint8_t *name, *sq, *ql, *aux, *end;
    const uint8_t* ops;          // n_ops operations of 4 bytes: the CIGAR field, or the CG tag's array
    int n_ops;
    int64_t rlen, qlen;          // 64-bit: a crafted CIGAR must not wrap the sums
    uint32_t op(int i) const { return uint32_t(le32(ops + size_t(i) * 4)); }
};

// The alignment records of one contig that the index names for [beg0, end0), in file order: open() is the preamble (file, header,
// reference id, index query), next() the record loop up to a record's fixed fields, lay_out() the rest of a record the consumer
// wants.  The consumer's own filter on the fixed fields sits between the two - a record it filters out is never laid out, so fields
// that lie raise no error there.  Every failure leaves `<who>: <what>` in err.
struct BamRegion {
    Bgzf bz;
    std::string who, err;
    int tid = -1;
    std::vector<std::string> names;      // reference names, when asked for
    std::vector<Chunk> chunks;
    std::vector<uint64_t> linear;        // the contig's linear index, when asked for
    int64_t beg0 = 0, end0 = 0;
    std::vector<uint8_t> rec;            // the record next() read last; a consumer that keeps a record swaps it out
    uint64_t rec_voff = 0;               // its virtual offset (of its block_size field)
    size_t ci = 0;                       // chunk being read
    bool in_chunk = false;

    bool fail(const char* fmt, ...) __attribute__((format(printf, 2, 3))) {
        char text[1024];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(text, sizeof text, fmt, ap);
        va_end(ap);
        err = who + ": " + text;
        return false;
    }
    bool open(const char* who_, const char* bam_path, const char* bai_path, const char* ctg_name, int64_t beg0_, int64_t end0_,
              bool want_linear, bool want_names, const PreInflated& pre = PreInflated{}) {
        who = who_;
        beg0 = beg0_;
        end0 = end0_;
        if (!bz.open(bam_path)) return fail("%s", bz.err.c_str());
        bz.pre = pre;
        // ---- header: the contig's reference id ----
        uint8_t h4[4];
        if (!(bz.read(h4, 4) && memcmp(h4, "BAM\1", 4) == 0)) return fail("%s is not a BAM file%s%s", bam_path, bz.err.empty() ? "" : ": ", bz.err.c_str());
        if (!bz.read(h4, 4)) return fail("truncated header");
        if (!(le32(h4) >= 0 && le32(h4) <= (1 << 28))) return fail("bad header text length");
        {
            std::vector<uint8_t> text(size_t(le32(h4)));
            if (!(text.empty() || bz.read(text.data(), text.size()))) return fail("truncated header text");
        }
        if (!bz.read(h4, 4)) return fail("truncated header");
        const int n_ref = le32(h4);
        if (n_ref < 0) return fail("bad reference count");
        std::vector<char> name;
        for (int r = 0; r < n_ref; ++r) {
            if (!bz.read(h4, 4)) return fail("truncated reference list");
            if (!(le32(h4) > 0 && le32(h4) <= 65536)) return fail("bad reference name length");
            name.resize(size_t(le32(h4)));
            if (!(bz.read(name.data(), name.size()) && bz.read(h4, 4))) return fail("truncated reference list");
            name.back() = 0;
            if (tid < 0 && strcmp(name.data(), ctg_name) == 0) tid = r;
            if (want_names) names.emplace_back(name.data());
        }
        if (tid < 0) return fail("contig %s not in the BAM header", ctg_name);
        // ---- index ----
        std::string ierr;
        const std::string idx = bai_path ? std::string(bai_path) : std::string(bam_path) + ".bai";
        if (!bai_query(idx.c_str(), tid, beg0, end0, &chunks, &ierr, want_linear ? &linear : nullptr)) return fail("%s", ierr.c_str());
        return true;
    }
    // The next record of the contig that starts before the region's end: 1 with the record in `rec` and its fixed fields in *r,
    // 0 when there is none (the chunks are read, the file ends, a record of a later contig or behind the region came), -1 on error.
    int next(BamRecord* r) {
        while (ci < chunks.size()) {
            if (!in_chunk) {
                if (!bz.seek(chunks[ci].beg)) { fail("seek into BAM failed: %s", bz.err.c_str()); return -1; }
                in_chunk = true;
            }
            if (bz.tell() >= chunks[ci].end) { ++ci; in_chunk = false; continue; }
            uint8_t h4[4];
            rec_voff = bz.settle();
            if (!bz.read(h4, 4)) {
                if (!bz.err.empty()) { fail("%s", bz.err.c_str()); return -1; }
                break;                                                          // clean end of the file
            }
            const int bsz = le32(h4);
            if (!(bsz >= 32 && bsz <= (1 << 28))) { fail("bad alignment block size %d", bsz); return -1; }
            rec.resize(size_t(bsz));
            if (!bz.read(rec.data(), rec.size())) { fail("truncated alignment record%s%s", bz.err.empty() ? "" : ": ", bz.err.c_str()); return -1; }
            const uint8_t* b = rec.data();
            const int rtid = le32(b);
            r->pos = le32(b + 4); r->l_name = b[8]; r->mapq = b[9];
            r->n_cig = b[12] | (b[13] << 8); r->flag = b[14] | (b[15] << 8); r->l_seq = le32(b + 16);
            r->next_ref = le32(b + 20); r->next_pos = le32(b + 24); r->tlen = le32(b + 28);
            if (rtid != tid) { if (rtid > tid || rtid < 0) break; continue; }
            if (r->pos >= end0) break;
            return 1;
        }
        ci = chunks.size();
        return 0;
    }
    // Lays out the record next() gave: false when it is shorter than its fields say.  CIGARs with more than 65535 operations live in
    // the CG:B,I tag; the CIGAR field then holds the placeholder <l_seq>S<ref_len>N of exactly two operations (SAM specification,
    // section 4.2.2), and the first field named CG of type B,I that lies wholly inside the record gives the operations.
    bool lay_out(BamRecord* r) {
        const size_t ls = size_t(std::max(r->l_seq, 0));
        const size_t need = 32 + size_t(r->l_name) + size_t(r->n_cig) * 4 + (ls + 1) / 2 + ls;
        if (r->l_seq < 0 || need > rec.size()) return fail("alignment record shorter than its fields");
        r->name = rec.data() + 32;
        const uint8_t* cg = r->name + r->l_name;
        r->sq = cg + size_t(r->n_cig) * 4;
        r->ql = r->sq + (ls + 1) / 2;
        r->aux = r->ql + ls;
        r->end = rec.data() + rec.size();
        r->ops = cg;
        r->n_ops = r->n_cig;
        if (r->n_cig == 2 && (le32(cg) & 15) == 4 && int(uint32_t(le32(cg)) >> 4) == r->l_seq && (le32(cg + 4) & 15) == 3) {
            const uint8_t* p = r->aux;
            for (AuxField f; aux_next(&p, r->end, &f);)
                if (f.type == 'B' && f.t0 == 'C' && f.t1 == 'G' && f.val[0] == 'I') {
                    r->ops = f.val + 5;
                    r->n_ops = int((f.len - 5) / 4);
                    break;
                }
        }
        r->rlen = r->qlen = 0;
        for (int i = 0; i < r->n_ops; ++i) {
            const uint32_t c = r->op(i);
            if (consumes_ref(int(c & 15))) r->rlen += int64_t(c >> 4);
            if (consumes_query(int(c & 15))) r->qlen += int64_t(c >> 4);
        }
        return true;
    }
    // What both pile-ups ask of a laid-out record: 1 when it enters, 0 when it is skipped (operations that do not add up to l_seq, no
    // reference base, wholly in front of the region), -1 when it ends past 2^31 - 1.
    int enters(const BamRecord& r) {
        if (r.qlen != r.l_seq || r.rlen == 0) return 0;
        if (int64_t(r.pos) + r.rlen > INT32_MAX) { fail("alignment at %d runs past 2^31 - 1", r.pos); return -1; }
        return int64_t(r.pos) + r.rlen > beg0;
    }
};

}  // namespace cto
