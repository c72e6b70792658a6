"""Panel-of-normals files for the tests: BGZF written block by block and its tabix index (.tbi) assembled field by field from the TBI
chapter of the SAM/htslib index specification (section 5.2 of SAMv1: magic "TBI\\1", n_ref, format, col_seq, col_beg, col_end, meta, skip,
l_nm, names; then per sequence the binning index - bins with their chunks of virtual offsets - and the 16 kb linear index), written as
BGZF itself.  Nothing here is shared with the reader in csrc/bam.cpp."""
import struct
import zlib

BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf_block(data, level=6):
    """one BGZF member: gzip header with the BC extra subfield (BSIZE = block size - 1), raw DEFLATE, CRC-32, ISIZE"""
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    payload = co.compress(data) + co.flush()
    bsize = 18 + len(payload) + 8
    return (b"\x1f\x8b\x08\x04" + b"\0\0\0\0" + b"\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, bsize - 1)
            + payload + struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data)))


def bgzf_compress(text, block=65280, eof=True, level=6):
    """-> (bytes, [(compressed offset, uncompressed start, length)] of the blocks); blocks cut every `block` bytes, lines cross them"""
    out, blocks, c = [], [], 0
    for u in range(0, len(text), block):
        b = bgzf_block(text[u:u + block], level)
        blocks.append((c, u, len(text[u:u + block])))
        out.append(b)
        c += len(b)
    if eof:
        out.append(BGZF_EOF)
    return b"".join(out), blocks


def voffset(blocks, u, total_len, end_comp):
    """virtual offset of uncompressed byte u: coffset << 16 | offset in the block; the end of a block is the start of the next one"""
    for coff, ustart, ulen in blocks:
        if ustart <= u < ustart + ulen:
            return coff << 16 | (u - ustart)
    return end_comp << 16


def reg2bin(beg, end):
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return base + (beg >> shift)
    return 0


def tbi_bytes(text, blocks, comp_len_without_eof):
    """the .tbi of a sorted VCF text (bytes) BGZF-compressed as `blocks`: format 2 (VCF), col_seq 1, col_beg 2, col_end 0, meta '#'"""
    names, per = [], {}
    u = 0
    for line in text.split(b"\n"):
        start, u = u, u + len(line) + 1
        if not line or line.startswith(b"#"):
            continue
        f = line.split(b"\t")
        ctg, beg = f[0], int(f[1]) - 1
        end = beg + max(1, len(f[3]))
        if ctg not in per:
            names.append(ctg)
            per[ctg] = ({}, [])
        vs = voffset(blocks, start, len(text), comp_len_without_eof)
        ve = voffset(blocks, min(u, len(text)), len(text), comp_len_without_eof)
        bins, linear = per[ctg]
        bins.setdefault(reg2bin(beg, end), []).append([vs, ve])
        for w in range(beg >> 14, ((end - 1) >> 14) + 1):
            while len(linear) <= w:
                linear.append(None)
            if linear[w] is None:
                linear[w] = vs
    l_nm = sum(len(n) + 1 for n in names)
    out = [b"TBI\x01", struct.pack("<iiiiiiii", len(names), 2, 1, 2, 0, ord("#"), 0, l_nm), b"".join(n + b"\0" for n in names)]
    for n in names:
        bins, linear = per[n]
        out.append(struct.pack("<i", len(bins)))
        for b in sorted(bins):
            merged = []
            for c in bins[b]:                               # records of a bin that follow each other share one chunk
                if merged and merged[-1][1] == c[0]:
                    merged[-1][1] = c[1]
                else:
                    merged.append(list(c))
            out.append(struct.pack("<Ii", b, len(merged)))
            for cb, ce in merged:
                out.append(struct.pack("<QQ", cb, ce))
        last = 0
        for i in range(len(linear)):                         # windows without a record take the next one's offset (htslib fills forward)
            if linear[i] is None:
                linear[i] = next((x for x in linear[i:] if x is not None), last)
            last = linear[i]
        out.append(struct.pack("<i", len(linear)))
        out.append(b"".join(struct.pack("<Q", x) for x in linear))
    raw = b"".join(out)
    return bgzf_compress(raw)[0]


def write_bgzf_vcf(path, text, with_tbi=True, block=65280):
    """`path` = BGZF of text (bytes) with the EOF block; `path`.tbi when asked"""
    comp, blocks = bgzf_compress(text, block=block)
    with open(path, "wb") as f:
        f.write(comp)
    if with_tbi:
        with open(path + ".tbi", "wb") as f:
            f.write(tbi_bytes(text, blocks, len(comp) - len(BGZF_EOF)))
    return len(comp)
