// One byte range of a BAM on its way through the device inflate (csrc/inflate.hip), for pipeline.hip's chunk producer and
// allelecount.hip: the range + its block table in page-locked memory, their device copy, the inflated blocks in their 256-byte
// aligned slots, the blocks' status words on both sides.  Call read, scan, inflate, and - once the caller has waited for what inflate
// queued - first_bad_status.  What a damaged or empty span means is the caller's to decide.
#pragma once
#include <algorithm>
#include "common.h"
#include "hip_buffers.h"
#include "run_files.h"

namespace cto {

struct InflatedSpan {
    PinBuf h_in, h_status;
    DevBuf d_in, d_out;                  // d_out: the inflated slots, the status words behind them at out_al
    size_t nbytes = 0, in_al = 0, cap = 0, out_al = 0;
    int64_t file_begin = 0, n = 0, out_bytes = 0;      // n: blocks in the table (or what cto_bgzf_scan returned instead)
    cto_bgzf_block* blocks() const { return reinterpret_cast<cto_bgzf_block*>(h_in.as<char>() + in_al); }

    // the bytes of the file, zero padding behind them; `who` goes in front of the error texts ("" or "name: ")
    int read(const char* path, int64_t begin, size_t bytes, const char* who) {
        nbytes = bytes; file_begin = begin; n = 0;
        in_al = (nbytes + CTO_BGZF_PAD + 255) / 256 * 256;
        cap = nbytes / 2048 + 64;
        if (const int rc = h_in.ensure(in_al + cap * sizeof(cto_bgzf_block))) return rc;
        const run_files::File f(path);
        CTO_REQUIRE(f.ok(), CTO_EINVAL, "%scannot open %s", who, path);
        CTO_REQUIRE(run_files::read_exact(f.fd, h_in.p, nbytes, file_begin), CTO_EINVAL, "%sshort read from %s", who, path);
        return CTO_OK;
    }
    // the block table behind the padding: cto_bgzf_scan's result, unchanged
    int64_t scan() {
        for (;;) {
            memset(h_in.as<char>() + nbytes, 0, in_al - nbytes);
            n = cto_bgzf_scan(h_in.as<uint8_t>(), nbytes, file_begin, blocks(), int64_t(cap), &out_bytes);
            if (n != CTO_ENOMEM || cap > (size_t(1) << 24)) return n;
            cap *= 8;                                              // many tiny blocks
            if (const int rc = h_in.grow_keeping(in_al + cap * sizeof(cto_bgzf_block), nbytes)) return n = rc;
        }
    }
    // device buffers, ONE copy up (bytes + table), cto_bgzf_inflate, the status words queued back
    int inflate(hipStream_t s) {
        const size_t tbl = size_t(n) * sizeof(cto_bgzf_block);
        out_al = (size_t(std::max<int64_t>(out_bytes, 256)) + 255) / 256 * 256;
        int rc;
        if ((rc = d_in.ensure(in_al + tbl)) || (rc = d_out.ensure(out_al + size_t(n) * 4)) || (rc = h_status.ensure(size_t(n) * 4))) return rc;
        CTO_HIP(hipMemcpyAsync(d_in.p, h_in.p, in_al + tbl, hipMemcpyHostToDevice, s));
        int* d_status = reinterpret_cast<int*>(d_out.as<char>() + out_al);
        if ((rc = cto_bgzf_inflate(d_in.p, reinterpret_cast<const cto_bgzf_block*>(d_in.as<char>() + in_al), int(n), d_out.p, d_status, s))) return rc;
        CTO_HIP(hipMemcpyAsync(h_status.p, d_status, size_t(n) * 4, hipMemcpyDeviceToHost, s));
        return CTO_OK;
    }
    int64_t first_bad_status() const {   // index of the first block that did not inflate (h_status has its code), -1: none
        for (int64_t b = 0; b < n; ++b) if (h_status.as<int>()[b] != 0) return b;
        return -1;
    }
};

}  // namespace cto
