// The HP class of the entered reads of a chunk on the device, shared by the front ends that read the tag there (aftally.hip: the AF
// tallies; hapwindows.hip: the haplotype windows).  A file-local kernel, like bam_records.h's: each source that includes this header
// gets its own copy.
#pragma once
#include "bam_records.h"

namespace {

// HP class of every entered read: the first HP field of an integer type -> 1, 2, 3 (the value 12) or 0; no such field -> 0.  The walk
// is bam_host.h's aux_next: it ends at a type it does not know and at a field that does not lie wholly inside the record.
__global__ void k_hp_class(const uint8_t* __restrict__ lin, const DevRead* __restrict__ reads, const int* __restrict__ rid, const Flags* fl,
                           uint8_t* __restrict__ hp) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= fl->n_valid) return;
    const DevRead r = reads[rid[j]];
    const uint8_t* rec = lin + r.off;
    const uint8_t* aend = rec + 4 + int64_t(int32_t(ld32(rec)));
    const uint8_t* aux = lin + r.qual_off + r.l_seq;
    int cls = 0;
    while (aend - aux >= 3) {
        const char t0 = char(aux[0]), t1 = char(aux[1]), ty = char(aux[2]);
        const uint8_t* v = aux + 3;
        const size_t left = size_t(aend - v);
        size_t len = 0;
        if (ty == 'A' || ty == 'c' || ty == 'C') len = 1;
        else if (ty == 's' || ty == 'S') len = 2;
        else if (ty == 'i' || ty == 'I' || ty == 'f') len = 4;
        else if (ty == 'Z' || ty == 'H') {
            while (len < left && v[len]) ++len;
            if (len == left) break;                                   // no NUL
            ++len;
        } else if (ty == 'B') {
            if (left < 5) break;
            const char sub = char(v[0]);
            len = 5 + size_t(ld32(v + 1)) * ((sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4);
        } else break;
        if (len > left) break;
        if (t0 == 'H' && t1 == 'P' && (ty == 'c' || ty == 'C' || ty == 's' || ty == 'S' || ty == 'i' || ty == 'I')) {
            long long val;
            if (ty == 'c') val = int8_t(v[0]);
            else if (ty == 'C') val = v[0];
            else if (ty == 's') val = int16_t(ld16(v));
            else if (ty == 'S') val = ld16(v);
            else if (ty == 'i') val = int32_t(ld32(v));
            else val = ld32(v);
            cls = val == 1 ? 1 : (val == 2 ? 2 : (val == 12 ? 3 : 0));
            break;
        }
        aux = v + len;
    }
    hp[j] = uint8_t(cls);
}

}  // namespace
