"""Test-only: the rules of csrc/contam.hip (a coverage, b keep, c merge, d output file) restated naively on plain lists, over BAMs read
with the Python reader of phase_tumor (not through the library), and the BAMs the tests run on, built with bamutil.write_bam."""
import random
import struct

import bamutil

from clairs_to_amd.phase_tumor import BgzfReader, BgzfWriter

COV_EXCL = 1796
CONSUMES_REF = (0, 2, 3, 7, 8)
NT16 = "=ACMGRSVTWYHKDBN"


# ------------------------------------------------------------------------------------------ reading
def read_bam(path):
    """-> (header bytes: magic .. reference list, refs [(name, length)], records [bytes, without the block_size field]) in file order"""
    rd = BgzfReader(str(path))
    try:
        head = rd.read(8)
        assert head[:4] == b"BAM\1"
        header = head + rd.read(struct.unpack_from("<i", head, 4)[0])
        n_ref = rd.read(4)
        header += n_ref
        refs = []
        for _ in range(struct.unpack("<i", n_ref)[0]):
            l_name = rd.read(4)
            name = rd.read(struct.unpack("<i", l_name)[0])
            ln = rd.read(4)
            header += l_name + name + ln
            refs.append((name.rstrip(b"\0").decode(), struct.unpack("<i", ln)[0]))
        recs = []
        while True:
            h4 = rd.read(4)
            if len(h4) < 4:
                break
            recs.append(rd.read(struct.unpack("<i", h4)[0]))
        return header, refs, recs
    finally:
        rd.close()


def fields(rec):
    tid, pos, l_name, mapq, bin_, n_cig, flag, l_seq, next_ref, next_pos, tlen = struct.unpack_from("<iiBBHHHiiii", rec, 0)
    name = rec[32:32 + max(l_name - 1, 0)]
    ops = list(struct.unpack_from("<%dI" % n_cig, rec, 32 + l_name))
    a0 = 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq
    return dict(tid=tid, pos=pos, l_name=l_name, mapq=mapq, bin=bin_, n_cig=n_cig, flag=flag, l_seq=l_seq, next_ref=next_ref, next_pos=next_pos,
                tlen=tlen, name=name, ops=ops, seq_at=32 + l_name + 4 * n_cig, aux_at=a0)


def real_ops(rec, f):
    """the CIGAR a reader uses: the field, or the CG:B,I tag under the placeholder <l_seq>S<n>N"""
    ops = f["ops"]
    if not (len(ops) == 2 and ops[0] == ((f["l_seq"] << 4) | 4) and (ops[1] & 15) == 3):
        return ops
    aux, i = rec[f["aux_at"]:], 0
    size = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
    while i + 3 <= len(aux):
        tag, ty = aux[i:i + 2], chr(aux[i + 2])
        i += 3
        if ty in size:
            i += size[ty]
        elif ty in "ZH":
            nul = aux.find(b"\0", i)
            if nul < 0:
                break
            i = nul + 1
        elif ty == "B":
            if i + 5 > len(aux):
                break
            sub, cnt = chr(aux[i]), struct.unpack_from("<I", aux, i + 1)[0]
            if tag == b"CG" and sub == "I" and i + 5 + 4 * cnt <= len(aux):
                return list(struct.unpack_from("<%dI" % cnt, aux, i + 5))
            i += 5 + cnt * size.get(sub, 4)
        else:
            break
    return ops


def ref_len(ops):
    return sum(c >> 4 for c in ops if (c & 15) in CONSUMES_REF)


# ------------------------------------------------------------------------------------------ rule a
def depth_array(recs, tid, length):
    """depth per position of contig `tid`, one list entry per base"""
    depth = [0] * length
    for rec in recs:
        f = fields(rec)
        if f["tid"] != tid or f["pos"] < 0 or (f["flag"] & COV_EXCL):
            continue
        for p in range(f["pos"], min(f["pos"] + ref_len(real_ops(rec, f)), length)):
            depth[p] += 1
    return depth


def coverage_table(path, ctg=None):
    """[dict(chrom, length, bases, min, max)] as bam_coverage gives it"""
    _, refs, recs = read_bam(path)
    out = []
    for tid, (name, length) in enumerate(refs):
        if ctg is not None and name != ctg:
            continue
        d = depth_array(recs, tid, length)
        out.append(dict(chrom=name, length=length, bases=sum(d), min=min(d) if d else 0, max=max(d) if d else 0))
    return out


# ------------------------------------------------------------------------------------------ rule b
def key24(name, seed=0):
    h = 0
    for i, b in enumerate(name):
        h = b if i == 0 else (h * 31 + b) & 0xffffffff
    k = (h ^ seed) & 0xffffffff
    k = (k + (~(k << 15) & 0xffffffff)) & 0xffffffff
    k ^= k >> 10
    k = (k + (k << 3)) & 0xffffffff
    k ^= k >> 6
    k = (k + (~(k << 11) & 0xffffffff)) & 0xffffffff
    k ^= k >> 16
    return k & 0xffffff


def keeps(k24, m):
    return k24 * 1000 < m * (1 << 24)


# ------------------------------------------------------------------------------------------ rules c and d
def merged_records(t_recs, n_recs, n_ref, m_t, m_n, seed=0, only_tid=None):
    """[(tid, record bytes)] of the output, in order"""
    out = []
    for tid in range(n_ref):
        if only_tid is not None and tid != only_tid:
            continue
        kept = []
        for src, (recs, m) in enumerate(((t_recs, m_t), (n_recs, m_n))):
            last = None
            for k, rec in enumerate(recs):
                f = fields(rec)
                if f["tid"] != tid:
                    continue
                assert last is None or f["pos"] >= last, "not coordinate-sorted"
                last = f["pos"]
                if f["pos"] >= 0 and keeps(key24(f["name"], seed), m):
                    kept.append((f["pos"], src, k, rec))
        kept.sort(key=lambda x: x[:3])                    # pos, tumour before normal, file order
        out += [(tid, x[3]) for x in kept]
    return out


def stream_of(header, merged):
    return header + b"".join(struct.pack("<i", len(rec)) + rec for _, rec in merged)


def write_expected(path, header, n_ref, merged, level=6):
    """the output file and its index by the rules of phase_tumor.haplotag_bam, through its BGZF writer"""
    wr = BgzfWriter(str(path), level)
    wr.write(header)
    bins, lin = [dict() for _ in range(n_ref)], [dict() for _ in range(n_ref)]
    for tid, rec in merged:
        f = fields(rec)
        vb = wr.tell()
        wr.write(struct.pack("<i", len(rec)) + rec)
        ve = wr.tell()
        beg = max(f["pos"], 0)
        end = max(beg + 1, f["pos"] + ref_len(f["ops"]))
        ch = bins[tid].setdefault(f["bin"], [])
        if ch and ch[-1][1] == vb:
            ch[-1][1] = ve
        else:
            ch.append([vb, ve])
        for w in range(beg >> 14, ((end - 1) >> 14) + 1):
            lin[tid].setdefault(w, vb)
    wr.close()
    out = b"BAI\1" + struct.pack("<i", n_ref)
    for tid in range(n_ref):
        out += struct.pack("<i", len(bins[tid]))
        for b, chunks in sorted(bins[tid].items()):
            out += struct.pack("<Ii", b, len(chunks)) + b"".join(struct.pack("<QQ", vb, ve) for vb, ve in chunks)
        n_intv = (max(lin[tid]) + 1) if lin[tid] else 0
        out += struct.pack("<i", n_intv)
        last = 0
        for w in range(n_intv):
            last = lin[tid].get(w, last)
            out += struct.pack("<Q", last)
    with open(str(path) + ".bai", "wb") as f:
        f.write(out)


def expected_bai(out_path, header, n_ref, merged):
    """the index of the file at out_path by the same rules, over the block offsets that file has: stream byte u lies in block u // 0xff00"""
    with open(str(out_path), "rb") as f:
        raw = f.read()
    coffs, o = [], 0
    while o < len(raw):
        coffs.append(o)
        o += struct.unpack_from("<H", raw, o + 16)[0] + 1

    def voff(u):
        return (coffs[u // 0xff00] << 16) | (u % 0xff00)
    bins, lin, u = [dict() for _ in range(n_ref)], [dict() for _ in range(n_ref)], len(header)
    for tid, rec in merged:
        f = fields(rec)
        vb, ve = voff(u), voff(u + 4 + len(rec))
        u += 4 + len(rec)
        beg = max(f["pos"], 0)
        end = max(beg + 1, f["pos"] + ref_len(f["ops"]))
        ch = bins[tid].setdefault(f["bin"], [])
        if ch and ch[-1][1] == vb:
            ch[-1][1] = ve
        else:
            ch.append([vb, ve])
        for w in range(beg >> 14, ((end - 1) >> 14) + 1):
            lin[tid].setdefault(w, vb)
    out = b"BAI\1" + struct.pack("<i", n_ref)
    for tid in range(n_ref):
        out += struct.pack("<i", len(bins[tid]))
        for b, chunks in sorted(bins[tid].items()):
            out += struct.pack("<Ii", b, len(chunks)) + b"".join(struct.pack("<QQ", vb, ve) for vb, ve in chunks)
        n_intv = (max(lin[tid]) + 1) if lin[tid] else 0
        out += struct.pack("<i", n_intv)
        last = 0
        for w in range(n_intv):
            last = lin[tid].get(w, last)
            out += struct.pack("<Q", last)
    return out


def inflated(path):
    """the whole inflated stream of a BGZF file, and whether it ends with the empty block"""
    rd = BgzfReader(str(path))
    try:
        parts = []
        while True:
            part = rd.read(1 << 20)
            if not part:
                break
            parts.append(part)
    finally:
        rd.close()
    with open(str(path), "rb") as f:
        raw = f.read()
    return b"".join(parts), raw[-28:] == bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def block_sizes(path):
    """the inflated size of every BGZF block of the file"""
    with open(str(path), "rb") as f:
        raw = f.read()
    out, o = [], 0
    while o < len(raw):
        bsize = struct.unpack_from("<H", raw, o + 16)[0] + 1
        out.append(struct.unpack_from("<I", raw, o + bsize - 4)[0])
        o += bsize
    return out


def view_rows(merged, refs, ctg, start, end):
    """the rows cto_bam_view gives for ctg:start-end (1-based, inclusive) over the records `merged`"""
    tid = [n for n, _ in refs].index(ctg)
    rows = []
    for t, rec in merged:
        f = fields(rec)
        ops = real_ops(rec, f)
        if t != tid or f["pos"] >= end or f["pos"] + max(ref_len(ops), 1) <= start - 1:
            continue
        seq = "".join(NT16[(rec[f["seq_at"] + (i >> 1)] >> ((~i & 1) << 2)) & 15] for i in range(f["l_seq"])) or "*"
        q = rec[f["seq_at"] + (f["l_seq"] + 1) // 2:f["aux_at"]]
        qual = "*" if not q or q[0] == 0xff else "".join(chr(min(x, 93) + 33) for x in q)
        rnext = "*" if f["next_ref"] < 0 else ("=" if f["next_ref"] == tid else refs[f["next_ref"]][0])
        rows.append("\t".join([f["name"].decode(), str(f["flag"]), ctg, str(f["pos"] + 1), str(f["mapq"]),
                               "".join("%d%s" % (c >> 4, "MIDNSHP=X"[c & 15]) for c in ops) or "*", rnext, str(f["next_pos"] + 1), str(f["tlen"]),
                               seq, qual]) + "\n")
    return rows


# ------------------------------------------------------------------------------------------ BAMs built by hand
HAND_REFS = [("c1", 100000), ("c2", 30000), ("c3", 500)]


def rd(name, ref, pos, cigar, flag=0, mapq=60, **kw):
    qlen = sum(n for op, n in cigar if op in bamutil.CONSUMES_QUERY)
    return dict(name=name, flag=flag, ref=ref, pos=pos, mapq=mapq, cigar=cigar, seq="ACGT" * (qlen // 4) + "ACGT"[:qlen % 4], qual=[30] * qlen, **kw)


def coverage_reads():
    """c1: a span clipped at the contig's end, a CG-tag CIGAR, rlen == 0, each of the four excluded flags, MAPQ 0, a read over more than
    two 16 kb windows, equal positions on both sides of a window edge; c2: no reads; c3: covered everywhere, min 2"""
    reads = [
        rd("plain", 0, 100, [("M", 500)]),
        rd("cgtag", 0, 1000, [("M", 300), ("D", 50), ("M", 200)], cg_tag=True),
        rd("norlen", 0, 2000, [("I", 50)]),
        rd("unmapped", 0, 2500, [("M", 100)], flag=4),
        rd("secondary", 0, 2600, [("M", 100)], flag=256),
        rd("qcfail", 0, 2700, [("M", 100)], flag=512),
        rd("duplicate", 0, 2800, [("M", 100)], flag=1024),
        rd("supplementary", 0, 2900, [("M", 100)], flag=2048),               # counts: not among mosdepth's default filters
        rd("mapq0", 0, 3000, [("M", 100)], mapq=0, flag=16),
        rd("long3", 0, 5000, [("M", 20000), ("D", 15000), ("M", 100)]),       # windows 0, 1 and 2: its end is carried twice
        rd("edge_a", 0, 16383, [("M", 10)]), rd("edge_b", 0, 16383, [("S", 5), ("M", 1)]),
        rd("edge_c", 0, 16384, [("M", 10)]), rd("edge_d", 0, 16384, [("M", 40000)]),
        rd("skip", 0, 50000, [("M", 10), ("N", 1000), ("M", 10)]),
        rd("clipped", 0, 99800, [("M", 500)]),
        rd("full1", 2, 0, [("M", 500)]), rd("full2", 2, 0, [("M", 600)]), rd("part", 2, 200, [("M", 100)]),
    ]
    assert [(r["ref"], r["pos"]) for r in reads] == sorted((r["ref"], r["pos"]) for r in reads)
    return reads


def mix_reads(kind, n=400, seed=5):
    """tumour ("t") or normal ("n") reads over HAND_REFS: pseudo-random short reads with ties between the sources at fixed positions, the
    normal without a record in c1's window 3 (48 - 64 kb) or on c3, the tumour with one record above 64 KB and a CG-tag read"""
    rng = random.Random(seed + (0 if kind == "t" else 1000))
    reads = []
    for i in range(n):
        ref = 0 if i % 10 else 1
        pos = rng.randrange(0, HAND_REFS[ref][1] - 300)
        if kind == "n" and ref == 0 and 48 * 1024 <= pos < 64 * 1024:
            continue
        reads.append(rd("%s%d" % (kind, i), ref, pos, [("M", rng.randrange(50, 250))], flag=16 * (i & 1)))
    for k, pos in enumerate((777, 777, 16383, 16384, 16384, 32768, 70000)):             # the same positions in both sources
        reads.append(rd("%stie%d" % (kind, k), 0, pos, [("M", 120)]))
    reads.append(rd("%smate" % kind, 0, 4000, [("M", 100)], flag=99))
    reads.append(rd("%smate" % kind, 0, 4300, [("M", 100)], flag=147))                   # mates share the name: kept or dropped together
    if kind == "t":
        reads.append(rd("tbig", 0, 3000, [("M", 70000)]))                                 # 4 + 32 + 5 + 4 + 35000 + 70000 bytes and its tags
        reads.append(rd("tcg", 0, 9000, [("M", 300), ("D", 50), ("M", 200)], cg_tag=True))
        reads.append(rd("tc3", 2, 10, [("M", 100)]))
    reads.sort(key=lambda r: (r["ref"], r["pos"]))
    return reads


def uniform_reads(kind, n, length, read_len, seed):
    """n reads of read_len bases each, wholly inside one contig of `length` bases, at sorted pseudo-random positions"""
    rng = random.Random(seed)
    pos = sorted(rng.randrange(0, length - read_len) for _ in range(n))
    return [rd("%s_%d" % (kind, i), 0, p, [("M", read_len)]) for i, p in enumerate(pos)]
