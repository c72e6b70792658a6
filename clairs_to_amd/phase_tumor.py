"""Phasing and haplotagging of one contig of a long-read tumour BAM: what run_clairs_to starts `longphase phase` and `longphase
haplotag` (or whatshap) for between STEP 3 and STEP 4.  The heterozygous SNP calls of select_hetero_snp_for_phasing go in; the phased
VCF and the haplotagged BAM that haplotype_filtering and cal_af_distribution read (HP, PS) come out.  No samtools, longphase or
whatshap is involved.  PARITY UNPINNED against those programs: the rules are this package's own (csrc/phase.hip lists them).

    python -m clairs_to_amd phase_tumor --tumor_bam_fn BAM [--bai_fn BAI] --vcf_fn <ctg>.vcf --ctg_name CTG
        --output_vcf_fn phased_vcf_output/tumor_phased_<ctg>.vcf.gz --output_bam_fn phased_bam_output/tumor_<ctg>.bam
        [--min_mq 20] [--link_span 8] [--where device|host]

One command instead of two, so the argv is its own; the file names are run_clairs_to's, and haplotype_filtering picks the BAM up through
its prefix mode (--tumor_bam_fn phased_bam_output/tumor_).

cto_phase_reads (csrc/phase.hip: the device path; csrc/bam.cpp: the host path) does the work on the reads: observations, link counts,
the phase pass, the reads' haplotypes.  What is here is host plumbing, in Python on zlib: the VCF rows with GT and PS rewritten, the
BAM copied record by record with HP / PS set, its BGZF blocks and its .bai."""
import ctypes as C
import gzip
import os
import struct
import sys
import zlib
from argparse import ArgumentParser

import numpy as np

MIN_MQ = 20
EXCL_FLAGS = 2316
LINK_SPAN = 8
PS_HEADER = '##FORMAT=<ID=PS,Number=1,Type=Integer,Description="Phase set identifier: the position of the first site of the phase block">\n'


def _default_where():
    import torch
    return "device" if torch.cuda.is_available() else "host"


# ------------------------------------------------------------------------------------------ the engine
def phase_reads(bam, ctg, pos, ref, alt, min_mq=MIN_MQ, excl_flags=EXCL_FLAGS, link_span=LINK_SPAN, where="device", bai=None, host_threads=0,
                stats=None):
    """cto_phase_reads at the 1-based, strictly ascending positions `pos` of contig `ctg` with their REF and ALT letters ->
    dict(phase int8 [n] (-1 unphased), ps int32 [n], link int32 [n, link_span, 2], voff uint64 [R] (the reads, in file order, by the
    virtual offset of their record), obs_off int64 [R + 1], obs int32 (site * 2 + allele), hp uint8 [R] (0 untagged), read_ps int32 [R]).
    where: "device" (HIP kernels on the current stream) or "host".  stats: a dict that receives the call's cto_phase_stats."""
    from ._lib import PhaseResult, PhaseStats, check, lib
    if where not in ("device", "host"):
        raise ValueError("where must be 'device' or 'host'")
    p = np.ascontiguousarray(pos, dtype=np.int32)
    n = len(p)
    if len(ref) != n or len(alt) != n:
        raise ValueError("one REF and one ALT letter per site")
    r = np.frombuffer("".join(ref).encode(), dtype=np.uint8) if n else np.zeros(0, dtype=np.uint8)
    a = np.frombuffer("".join(alt).encode(), dtype=np.uint8) if n else np.zeros(0, dtype=np.uint8)
    if len(r) != n or len(a) != n:
        raise ValueError("REF and ALT are one ASCII letter each")
    phase = np.full(n, -1, dtype=np.int8)
    ps = np.zeros(n, dtype=np.int32)
    link = np.zeros((n, int(link_span), 2), dtype=np.int32)
    st, res = PhaseStats(), C.POINTER(PhaseResult)()
    stream = None
    if where == "device":
        from ._lib import current_stream_ptr
        stream = C.c_void_p(current_stream_ptr())
    check(lib.cto_phase_reads(str(bam).encode(), str(bai).encode() if bai else None, ctg.encode(), p.ctypes.data, r.ctypes.data, a.ctypes.data, n,
                              int(min_mq), int(excl_flags), int(link_span), 1 if where == "device" else 0, int(host_threads), stream,
                              phase.ctypes.data, ps.ctypes.data, link.ctypes.data, C.byref(res), C.byref(st)))
    try:
        v = res.contents

        def arr(ptr, m, dt):
            return np.frombuffer(C.string_at(ptr, m * np.dtype(dt).itemsize), dtype=dt).copy() if m else np.zeros(0, dtype=dt)
        out = dict(phase=phase, ps=ps, link=link, voff=arr(v.voff, v.n_reads, "<u8"), obs_off=arr(v.obs_off, v.n_reads + 1, "<i8"),
                   obs=arr(v.obs, v.n_obs, "<i4"), hp=arr(v.hp, v.n_reads, "u1"), read_ps=arr(v.ps, v.n_reads, "<i4"))
    finally:
        lib.cto_phase_result_free(res)
    if stats is not None:
        for name, _ in PhaseStats._fields_:
            stats[name] = stats.get(name, 0) + getattr(st, name)
    return out


# ------------------------------------------------------------------------------------------ VCF
def _open_text(fn):
    with open(fn, "rb") as f:
        gz = f.read(2) == b"\x1f\x8b"
    return gzip.open(fn, "rt") if gz else open(fn)


def read_sites(vcf_fn, ctg):
    """-> (rows: every line of the file, sites: [(row index, pos, REF, ALT)]) - the rows of `ctg` with one REF and one ALT letter and ten
    columns, at strictly ascending positions (a row that repeats or falls behind an earlier position is no site: it stays as it is)"""
    with _open_text(vcf_fn) as f:
        rows = f.readlines()
    sites, last = [], 0
    for i, row in enumerate(rows):
        if row.startswith("#") or not row.strip():
            continue
        c = row.rstrip("\n").split("\t")
        if len(c) < 10 or c[0] != ctg or len(c[3]) != 1 or len(c[4]) != 1:
            continue
        pos = int(c[1])
        if pos <= last or pos >= 2 ** 31:
            continue
        sites.append((i, pos, c[3], c[4]))
        last = pos
    return rows, sites


def phased_rows(rows, sites, phase, ps):
    """the rows with GT rewritten to 0|1 (ALT on haplotype 2) or 1|0 and PS appended to FORMAT and the sample at the phased sites; one
    ##FORMAT line for PS in front of #CHROM"""
    out = list(rows)
    for (i, _, _, _), ph, p in zip(sites, phase, ps):
        if ph < 0:
            continue
        c = out[i].rstrip("\n").split("\t")
        fmt, smp = c[8].split(":"), c[9].split(":")
        smp += [""] * (len(fmt) - len(smp))
        smp[fmt.index("GT")] = "%d|%d" % (ph, 1 - ph)
        if "PS" in fmt:
            smp[fmt.index("PS")] = str(int(p))
        else:
            fmt.append("PS")
            smp.append(str(int(p)))
        c[8], c[9] = ":".join(fmt), ":".join(smp)
        out[i] = "\t".join(c) + "\n"
    if not any(r.startswith("##FORMAT=<ID=PS,") for r in out):
        at = next((i for i, r in enumerate(out) if r.startswith("#CHROM")), 0)
        out.insert(at, PS_HEADER)
    return out


def write_vcf_gz(fn, rows):
    with open(fn, "wb") as f:
        with gzip.GzipFile(filename="", fileobj=f, mode="wb", mtime=0) as g:      # no name, no time: the same rows give the same bytes
            g.write("".join(rows).encode())


# ------------------------------------------------------------------------------------------ BAM
class BgzfReader(object):
    """the inflated stream of a BGZF file, read in order; tell() names the next byte as the library does: by the block that holds it"""

    def __init__(self, path):
        self.f = open(path, "rb")
        self.coff = self.next_coff = 0
        self.block, self.upos = b"", 0

    def close(self):
        self.f.close()

    def _load(self, coff):
        self.f.seek(coff)
        head = self.f.read(18)
        if len(head) == 0:
            return False
        if len(head) < 18 or head[:4] != b"\x1f\x8b\x08\x04":
            raise ValueError("phase_tumor: not a BGZF block at offset %d" % coff)
        xlen = struct.unpack_from("<H", head, 10)[0]
        extra = head[12:] + self.f.read(xlen - 6)
        bsize, i = 0, 0
        while i + 4 <= len(extra):
            slen = struct.unpack_from("<H", extra, i + 2)[0]
            if extra[i:i + 2] == b"BC" and slen == 2:
                bsize = struct.unpack_from("<H", extra, i + 4)[0] + 1
            i += 4 + slen
        if bsize == 0:
            raise ValueError("phase_tumor: BGZF block without BC subfield at offset %d" % coff)
        rest = self.f.read(bsize - 12 - xlen)
        if len(rest) != bsize - 12 - xlen:
            raise ValueError("phase_tumor: truncated BGZF block at offset %d" % coff)
        data = zlib.decompress(rest[:-8], -15)
        crc, isize = struct.unpack("<II", rest[-8:])
        if len(data) != isize or (zlib.crc32(data) & 0xffffffff) != crc:
            raise ValueError("phase_tumor: BGZF block at offset %d fails its CRC-32" % coff)
        self.coff, self.next_coff, self.block, self.upos = coff, coff + bsize, data, 0
        return True

    def seek(self, voff):
        self._load(voff >> 16)
        self.upos = voff & 0xffff

    def tell(self):
        while self.upos >= len(self.block):
            if not self._load(self.next_coff):
                break
        return (self.coff << 16) | self.upos

    def read(self, n):
        out = []
        while n > 0:
            if self.upos >= len(self.block):
                if not self._load(self.next_coff):
                    break
                continue
            part = self.block[self.upos:self.upos + n]
            self.upos += len(part)
            n -= len(part)
            out.append(part)
        return b"".join(out)


class BgzfWriter(object):
    """BGZF blocks of up to 0xff00 inflated bytes through zlib; tell() is the virtual offset of the next byte"""
    PAYLOAD = 0xff00

    def __init__(self, path, level=6):
        self.f, self.level = open(path, "wb"), level
        self.coff, self.buf = 0, bytearray()

    def _flush(self):
        data = bytes(self.buf[:self.PAYLOAD])
        del self.buf[:self.PAYLOAD]
        co = zlib.compressobj(self.level, zlib.DEFLATED, -15)
        comp = co.compress(data) + co.flush()
        if len(comp) + 26 > 65536:                      # does not happen at 0xff00 bytes unless the data cannot be compressed at all
            co = zlib.compressobj(0, zlib.DEFLATED, -15)
            comp = co.compress(data) + co.flush()
        block = struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(comp) + 25) + comp + struct.pack(
            "<II", zlib.crc32(data) & 0xffffffff, len(data))
        self.f.write(block)
        self.coff += len(block)

    def tell(self):
        return (self.coff << 16) | len(self.buf)

    def write(self, data):
        self.buf += data
        while len(self.buf) >= self.PAYLOAD:
            self._flush()

    def close(self):
        if self.buf:
            self._flush()
        self._flush()                                   # the empty block that ends the file
        self.f.close()


class BatchBgzfWriter(object):
    """The same blocks through csrc/deflate.hip (where: "device", or "host" for its host restatement), up to BATCH of them per
    cto_bgzf_deflate call.  A block's file offset is not known while it waits for its batch, so tell() names the next byte in
    block-index space, (block index << 16) | offset in the block; file_voff() turns such an offset into a virtual file offset once
    close() has written everything."""
    PAYLOAD = 0xff00
    BATCH = 256

    def __init__(self, path, where="device", device=None):
        self.f, self.where, self.device = open(path, "wb"), where, device
        self.buf, self.n_done, self.block_off, self.coff = bytearray(), 0, [], 0

    def _code(self, n_bytes):
        from .bgzf import deflate_blocks
        data = bytes(self.buf[:n_bytes])
        del self.buf[:n_bytes]
        blocks, sizes = deflate_blocks(data, self.where, self.device)
        for sz in sizes:
            self.block_off.append(self.coff)
            self.coff += int(sz)
        self.n_done += len(sizes)
        self.f.write(blocks)

    def tell(self):
        return ((self.n_done + len(self.buf) // self.PAYLOAD) << 16) | (len(self.buf) % self.PAYLOAD)

    def write(self, data):
        self.buf += data
        if len(self.buf) >= self.BATCH * self.PAYLOAD:
            self._code(len(self.buf) // self.PAYLOAD * self.PAYLOAD)

    def close(self):
        from .bgzf import BGZF_EOF
        if self.buf:
            self._code(len(self.buf))
        self.block_off.append(self.coff)                # the empty block that ends the file
        self.f.write(BGZF_EOF)
        self.f.close()

    def file_voff(self, v):
        return (self.block_off[v >> 16] << 16) | (v & 0xffff)


_AUX_SIZE = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}


def strip_tags(aux, drop=(b"HP", b"PS")):
    """the auxiliary area without the fields named in `drop` (of any type); what cannot be walked stays as it is"""
    out, i, n = [], 0, len(aux)
    while i + 3 <= n:
        ty = chr(aux[i + 2])
        j = i + 3
        if ty in _AUX_SIZE:
            j += _AUX_SIZE[ty]
        elif ty in "ZH":
            nul = aux.find(b"\0", j)
            if nul < 0:
                break
            j = nul + 1
        elif ty == "B" and j + 5 <= n:
            j += 5 + struct.unpack_from("<I", aux, j + 1)[0] * _AUX_SIZE.get(chr(aux[j]), 4)
        else:
            break
        if j > n:
            break
        if aux[i:i + 2] not in drop:
            out.append(aux[i:j])
        i = j
    out.append(aux[i:])
    return b"".join(out)


def _first_offset(bai_fn, tid):
    """the smallest virtual offset the index names for reference `tid`; None when it names none"""
    with open(bai_fn, "rb") as f:
        b = f.read()
    if b[:4] != b"BAI\1":
        raise ValueError("phase_tumor: %s is not a BAI index" % bai_fn)
    n_ref, o, first = struct.unpack_from("<i", b, 4)[0], 8, None
    for r in range(min(n_ref, tid + 1)):
        n_bin = struct.unpack_from("<i", b, o)[0]
        o += 4
        for _ in range(n_bin):
            bin_, n_chunk = struct.unpack_from("<Ii", b, o)
            o += 8
            if r == tid and bin_ != 37450:
                for k in range(n_chunk):
                    beg = struct.unpack_from("<Q", b, o + 16 * k)[0]
                    first = beg if first is None else min(first, beg)
            o += 16 * n_chunk
        n_intv = struct.unpack_from("<i", b, o)[0]
        o += 4 + 8 * n_intv
    return first


_CONSUMES_REF = (0, 2, 3, 7, 8)


def haplotag_bam(bam_fn, bai_fn, ctg, tags, out_fn, level=6, deflate="zlib", device=None):
    """Writes out_fn and out_fn + '.bai': the header of bam_fn, verbatim, and every record of contig `ctg` in file order - the ones that
    did not enter the phasing too - without the HP and PS fields it came with, and with HP:i / PS:i appended where tags names its
    virtual offset: {voff: (hp, ps)}.  The index: bins from the records' own bin field, 16 kb linear index.  deflate: "zlib" (level
    `level`), or "device" / "host" for csrc/deflate.hip and its host restatement (the same bytes from both).  -> (records, tagged)"""
    if deflate not in ("zlib", "device", "host"):
        raise ValueError("phase_tumor: deflate must be zlib, device or host")
    rd = BgzfReader(bam_fn)
    try:
        head = rd.read(8)
        if head[:4] != b"BAM\1":
            raise ValueError("phase_tumor: %s is not a BAM file" % bam_fn)
        header = head + rd.read(struct.unpack_from("<i", head, 4)[0])
        n_ref = struct.unpack("<i", rd.read(4))[0]
        header += struct.pack("<i", n_ref)
        tid = -1
        for r in range(n_ref):
            l_name = rd.read(4)
            name = rd.read(struct.unpack("<i", l_name)[0])
            header += l_name + name + rd.read(4)
            if tid < 0 and name.rstrip(b"\0").decode() == ctg:
                tid = r
        if tid < 0:
            raise ValueError("phase_tumor: contig %s not in the BAM header" % ctg)
        wr = BgzfWriter(out_fn, level) if deflate == "zlib" else BatchBgzfWriter(out_fn, deflate, device)
        wr.write(header)
        bins, lin = {}, {}
        n_rec = n_tag = 0
        first = _first_offset(bai_fn, tid)
        if first is not None:
            rd.seek(first)
            while True:
                voff = rd.tell()
                h4 = rd.read(4)
                if len(h4) < 4:
                    break
                rec = rd.read(struct.unpack("<i", h4)[0])
                rtid, pos, l_name, _mapq, bin_, n_cig, _flag, l_seq = struct.unpack_from("<iiBBHHHi", rec, 0)
                if rtid != tid:
                    if rtid > tid or rtid < 0:
                        break
                    continue
                a0 = 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq
                aux = strip_tags(rec[a0:])
                t = tags.get(voff)
                if t is not None and t[0]:
                    aux += b"HPi" + struct.pack("<i", t[0]) + b"PSi" + struct.pack("<i", t[1])
                    n_tag += 1
                rec = rec[:a0] + aux
                vb = wr.tell()
                wr.write(struct.pack("<i", len(rec)) + rec)
                ve = wr.tell()
                n_rec += 1
                rlen = sum(c >> 4 for c in struct.unpack_from("<%dI" % n_cig, rec, 32 + l_name) if (c & 15) in _CONSUMES_REF)
                beg = max(pos, 0)
                end = max(beg + 1, pos + rlen)
                ch = bins.setdefault(bin_, [])
                if ch and ch[-1][1] == vb:
                    ch[-1][1] = ve
                else:
                    ch.append([vb, ve])
                for w in range(beg >> 14, ((end - 1) >> 14) + 1):
                    lin.setdefault(w, vb)
        wr.close()
        if deflate != "zlib":                           # block-index space -> file offsets, now that every block has its size
            bins = {b: [[wr.file_voff(vb), wr.file_voff(ve)] for vb, ve in chunks] for b, chunks in bins.items()}
            lin = {w: wr.file_voff(v) for w, v in lin.items()}
    finally:
        rd.close()
    out = b"BAI\1" + struct.pack("<i", n_ref)
    for r in range(n_ref):
        if r != tid:
            out += struct.pack("<ii", 0, 0)
            continue
        out += struct.pack("<i", len(bins))
        for b, chunks in sorted(bins.items()):
            out += struct.pack("<Ii", b, len(chunks)) + b"".join(struct.pack("<QQ", vb, ve) for vb, ve in chunks)
        n_intv = (max(lin) + 1) if lin else 0
        out += struct.pack("<i", n_intv)
        last = 0
        for w in range(n_intv):
            last = lin.get(w, last)
            out += struct.pack("<Q", last)
    with open(out_fn + ".bai", "wb") as f:
        f.write(out)
    return n_rec, n_tag


# ------------------------------------------------------------------------------------------ the step
def phase_tumor(args):
    where = args.where or _default_where()
    bai = args.bai_fn or args.tumor_bam_fn + ".bai"
    rows, sites = read_sites(args.vcf_fn, args.ctg_name)
    stats = {}
    res = phase_reads(args.tumor_bam_fn, args.ctg_name, [s[1] for s in sites], [s[2] for s in sites], [s[3] for s in sites], min_mq=args.min_mq,
                      link_span=args.link_span, where=where, bai=bai, host_threads=args.threads or 0, stats=stats)
    for fn in (args.output_vcf_fn, args.output_bam_fn):
        if os.path.dirname(fn):
            os.makedirs(os.path.dirname(fn), exist_ok=True)
    write_vcf_gz(args.output_vcf_fn, phased_rows(rows, sites, res["phase"], res["ps"]))
    tags = {int(v): (int(h), int(p)) for v, h, p in zip(res["voff"], res["hp"], res["read_ps"]) if h}
    deflate = getattr(args, "deflate", None) or "zlib"
    n_rec, n_tag = haplotag_bam(args.tumor_bam_fn, bai, args.ctg_name, tags, args.output_bam_fn, deflate=deflate)
    print("[INFO] phase_tumor %s: %d of %d sites phased in %d blocks; %d of %d reads tagged (%d entered); %s path" % (
        args.ctg_name, int((res["phase"] >= 0).sum()), len(sites), stats.get("n_phase_blocks", 0), n_tag, n_rec, len(res["voff"]), where))
    if deflate != "zlib":
        print("[INFO] phase_tumor %s: BGZF deflate of the output BAM: %s" % (args.ctg_name, deflate))
    return res


def build_parser():
    ap = ArgumentParser(prog="phase_tumor", description="Phase the heterozygous SNP calls of one contig and haplotag the tumour BAM's reads "
                        "(in place of longphase / whatshap phase + haplotag)")
    ap.add_argument("--tumor_bam_fn", type=str, default=None, help="Sorted tumour BAM, with its index")
    ap.add_argument("--bai_fn", type=str, default=None, help="The BAM's index, default: <tumor_bam_fn>.bai")
    ap.add_argument("--vcf_fn", type=str, default=None, help="The contig's heterozygous SNP calls (select_hetero_snp_for_phasing's <ctg>.vcf), plain or gzip")
    ap.add_argument("--ctg_name", type=str, default=None, help="The name of the sequence to be processed")
    ap.add_argument("--output_vcf_fn", type=str, default=None, help="Phased VCF, gzip-compressed (phased_vcf_output/tumor_phased_<ctg>.vcf.gz).  No "
                    "tabix index is written: nothing in this package needs one")
    ap.add_argument("--output_bam_fn", type=str, default=None, help="Haplotagged BAM (phased_bam_output/tumor_<ctg>.bam); its .bai is written beside it")
    ap.add_argument("--min_mq", type=int, default=MIN_MQ, help="Reads below this mapping quality take no part, default: %(default)d")
    ap.add_argument("--link_span", type=int, default=LINK_SPAN, help="How many sites ahead a site is linked to, default: %(default)d")
    ap.add_argument("--where", type=str, default=None, choices=("device", "host"), help="Where the reads are phased, default: device when there is one")
    ap.add_argument("--threads", type=int, default=0, help="Threads of the host path, default: one per core, at most 32")
    ap.add_argument("--deflate", type=str, default="zlib", choices=("zlib", "device", "host"), help="The coder of the output BAM's BGZF blocks: "
                    "zlib level 6, the device coder (csrc/deflate.hip), or its host restatement, default: %(default)s")
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(sys.argv[1:] if argv is None else argv)
    for name in ("tumor_bam_fn", "vcf_fn", "ctg_name", "output_vcf_fn", "output_bam_fn"):
        if getattr(args, name) is None:
            sys.exit("phase_tumor: --%s is required" % name)
    from ._lib import CtoError
    try:
        phase_tumor(args)
    except (CtoError, ValueError) as e:
        sys.exit("phase_tumor: %s" % e)


if __name__ == "__main__":
    main()
