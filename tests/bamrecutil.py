"""Test-only: the BAM files that take the record front end (csrc/bam_records.h on the device, BamRegion of csrc/bam_host.h on the host)
away from the one record shape tests/bamutil.py:write_bam gives by default - auxiliary areas of every layout around CG:B,I, BGZF
blocks at the seams of the CRC-32 slices, fixed fields at their gates, records whose fields lie - and the naive expectations for them.
Shared by tests/test_bam_records.py (host) and tests/test_gpu_bam_records.py (device); every file is written once per process.
The walk rules follow the SAM specification as bamutil.effective_cigar restates it; PARITY UNPINNED against htslib (not installed)."""
import functools
import hashlib
import os
import struct
import tempfile
import zlib

import numpy as np

from allelecountutil import PARAMS, naive_counts
from bamutil import CONSUMES_QUERY, _cigar_bytes, _record, effective_cigar, ref_len_of, write_bam

# name -> (min_bq, min_mq, req_flags, excl_flags): the Verdict step's, and nothing filtered at all
AUX_PARAMS = {"verdict": PARAMS["verdict"], "zero": (0, 0, 0, 0)}


@functools.lru_cache(maxsize=None)
def _dir():
    return tempfile.mkdtemp(prefix="bam_records_")


def query_len_of(cigar):
    return sum(n for op, n in cigar if op in CONSUMES_QUERY)


# ------------------------------------------------------------------------------------------------ naive expectations
def effective_reads(reads):
    """what a reader makes of the records: each with its effective CIGAR; records that are no placed alignment (pos < 0, no
    reference) and the pre-encoded ones are left out"""
    return [dict(r, cigar=effective_cigar(r)) for r in reads if "raw" not in r and r["ref"] >= 0 and r["pos"] >= 0]


def naive(reads, ref_index, positions, min_bq, min_mq, req_flags, excl_flags):
    out = naive_counts(effective_reads(reads), ref_index, positions, min_bq, min_mq, req_flags, excl_flags)
    out.setflags(write=False)
    return out


def naive_entered(reads, ref_index, positions, min_bq, min_mq, req_flags, excl_flags):
    """how many reads enter the pile-up of positions[0]..positions[-1] (1-based): the rules at the top of csrc/allelecount.hip"""
    n = 0
    for r in effective_reads(reads):
        f = r["flag"]
        if r["ref"] != ref_index or r["mapq"] < min_mq or (f & excl_flags) or (f & req_flags) != req_flags or (f & 1796):
            continue
        if (req_flags & 2) and bool(f & 32) == bool(f & 16):
            continue
        rl = ref_len_of(r["cigar"])
        if not r["cigar"] or not r["seq"] or rl == 0 or query_len_of(r["cigar"]) != len(r["seq"]):
            continue
        n += r["pos"] + 1 <= positions[-1] and r["pos"] + rl >= positions[0]
    return n


def blame(positions, got, want, named_reads):
    """the name of the read among `named_reads` [(name, read)] that covers the first position where got and want differ"""
    bad = np.nonzero((np.asarray(got) != np.asarray(want)).any(axis=1))[0]
    if len(bad) == 0:
        return ""
    p = positions[int(bad[0])]
    names = [n for n, r in named_reads if r["pos"] <= p <= r["pos"] + max(1, ref_len_of(effective_cigar(r))) + 6]
    return "first difference at %d (got %s, want %s), under: %s" % (p, got[bad[0]], want[bad[0]], ", ".join(names) or "no layout read")


def bam_digests(path):
    """(sha256 of the .bam and .bai bytes, sha256 of what they say whatever the compressor: every block's inflated bytes, and the
    index with each virtual offset's file offset replaced by its block's number)"""
    raw = open(path, "rb").read()
    offs, o, h = {}, 0, hashlib.sha256()
    while o < len(raw):
        bsize = struct.unpack_from("<H", raw, o + 16)[0] + 1
        data = zlib.decompressobj(-15).decompress(raw[o + 18:o + bsize - 8])
        assert struct.unpack_from("<II", raw, o + bsize - 8) == (zlib.crc32(data) & 0xffffffff, len(data))
        offs[o] = len(offs)
        h.update(struct.pack("<I", len(data)) + data)
        o += bsize
    offs[o] = len(offs)
    bai = open(path + ".bai", "rb").read()
    h.update(bai[:8])
    n_ref, p = struct.unpack_from("<i", bai, 4)[0], 8
    v = lambda x: struct.pack("<QH", offs[x >> 16], x & 0xffff)
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", bai, p)[0]
        h.update(bai[p:p + 4])
        p += 4
        for _ in range(n_bin):
            n_chunk = struct.unpack_from("<Ii", bai, p)[1]
            h.update(bai[p:p + 8])
            p += 8
            for _ in range(2 * n_chunk):
                h.update(v(struct.unpack_from("<Q", bai, p)[0]))
                p += 8
        n_intv = struct.unpack_from("<i", bai, p)[0]
        h.update(bai[p:p + 4])
        p += 4
        for _ in range(n_intv):
            h.update(v(struct.unpack_from("<Q", bai, p)[0]))
            p += 8
    assert p == len(bai)
    return hashlib.sha256(raw + bai).hexdigest(), h.hexdigest()


# ------------------------------------------------------------------------------------------------ reads
def _seq(rng, n):
    return "".join(rng.choice(list("ACGT"), size=n))


def _read(rng, name, ref, pos, cigar, flag=0, mapq=60, l_seq=None, **kw):
    n = query_len_of(cigar) if l_seq is None else l_seq
    return dict(name=name, flag=flag, ref=ref, pos=pos, mapq=mapq, cigar=cigar, seq=_seq(rng, n),
                qual=[int(q) for q in rng.integers(10, 41, size=n)], **kw)


def _long_cigar(rng, first=None):
    """at least five operations with an I and a D, no N, 40 to 60 query bases"""
    while True:
        ops = [first or ("S", int(rng.integers(1, 5))), ("M", int(rng.integers(8, 16))), ("I", int(rng.integers(1, 4))),
               (str(rng.choice(list("M=X"))), int(rng.integers(8, 14))), ("D", int(rng.integers(1, 6))), ("M", int(rng.integers(8, 16)))]
        if rng.random() < 0.5:
            ops += [("I", 1), ("M", int(rng.integers(3, 9)))]
        if 40 <= query_len_of(ops) <= 60:
            return ops


def _tag(name, ty, payload=b""):
    return name.encode() + ty.encode() + payload


def _b_array(name, sub, values):
    fmt = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}[sub]
    return _tag(name, "B", sub.encode() + struct.pack("<I", len(values)) + struct.pack("<%d%s" % (len(values), fmt), *values))


def _cg(cigar, name="CG"):
    return _tag(name, "B", b"I" + struct.pack("<I", len(cigar)) + _cigar_bytes(cigar))


_SCALARS = {"A": b"q", "c": struct.pack("<b", -3), "C": struct.pack("<B", 200), "s": struct.pack("<h", -300), "S": struct.pack("<H", 60000),
            "i": struct.pack("<i", -70000), "I": struct.pack("<I", 4000000000), "f": struct.pack("<f", 1.5)}

AUX_CTG, AUX_STEP, AUX_FIRST = "aux", 200, 300


def _aux_layouts(rng):
    """[(layout name, extras of its read dict beyond the real `cigar`, taken)]: taken = the CG tag's operations are the record's"""
    L = []

    def add(name, aux, taken=True, cigar=None, **kw):
        real = cigar or _long_cigar(rng)
        L.append((name, dict(cigar=real, aux=aux(real), **kw), taken))
    nm, xa = _tag("NM", "i", struct.pack("<i", 3)), _tag("XA", "Z", b"chr9,+1,5M;\0")
    add("cg_only", lambda c: _cg(c))
    add("cg_first", lambda c: _cg(c) + nm + xa)
    add("cg_last", lambda c: nm + xa + _cg(c))
    for ty in "AcCsSiIf":
        add("scalar_%s" % ty, lambda c, ty=ty: _tag("X" + ty, ty, _SCALARS[ty]) + _cg(c))
    add("scalars_all", lambda c: b"".join(_tag("Y" + ty, ty, _SCALARS[ty]) for ty in "AcCsSiIf") + _cg(c))
    add("z_empty", lambda c: _tag("XZ", "Z", b"\0") + _cg(c))
    add("z_300", lambda c: _tag("XZ", "Z", bytes(33 + k % 90 for k in range(300)) + b"\0") + _cg(c))
    add("h_before", lambda c: _tag("XH", "H", b"1AE301\0") + _cg(c))
    for sub in "cCsSiIf":
        for cnt in (0, 1, 7):
            vals = [1.25 * k for k in range(cnt)] if sub == "f" else [(k * 37 + 5) % 100 for k in range(cnt)]
            add("b_%s_%d" % (sub, cnt), lambda c, sub=sub, vals=vals: _b_array("XB", sub, vals) + _cg(c))
    # a B,I array of another name in front, the same count: its deletion is three bases longer, everything behind it would shift
    shifted = lambda c: [(op, n + 3) if op == "D" else (op, n) for op, n in c]
    add("xi_bi_before", lambda c: _cg(shifted(c), name="XI") + _cg(c))
    # ---- a CG tag that must not be taken: the placeholder stands
    add("cg_sub_i", lambda c: _tag("CG", "B", b"i" + struct.pack("<I", len(c)) + _cigar_bytes(c)), taken=False)
    add("cg_z", lambda c: _tag("CG", "Z", b"20M2I20M\0"), taken=False)
    add("cg_overrun", lambda c: _tag("CG", "B", b"I" + struct.pack("<I", len(c) + 1) + _cigar_bytes(c)), taken=False)
    add("unknown_type", lambda c: _tag("XQ", "?", b"\1") + _cg(c), taken=False)
    # no NUL of the Z's own: it runs into the CG tag's count (a 32-bit count always has a zero byte); what is left of the tag
    # reads as a field of type '4' (the low byte of 3S), unknown, and the walk ends
    add("z_no_nul", lambda c: _tag("XZ", "Z", b"unterminated") + _cg(c), taken=False, cigar=_long_cigar(rng, first=("S", 3)))
    add("no_aux", lambda c: b"", taken=False)
    # the record's last tag a Z with no zero byte behind it: it runs to the record's end; a B whose five header bytes do not fit
    add("z_to_record_end", lambda c: nm + _tag("XZ", "Z", b"never terminated"), taken=False)
    add("b_header_cut", lambda c: nm + _tag("CG", "B", b"I" + struct.pack("<H", len(c))), taken=False)
    L = [(n, dict(e, cigar_field=[("S", query_len_of(e["cigar"])), ("N", ref_len_of(e["cigar"]))]), t) for n, e, t in L]
    # ---- a field that is no placeholder: the valid CG behind it is ignored
    c = _long_cigar(rng)
    L.append(("field_three_ops", dict(cigar=c, aux=_cg(c), cigar_field=[("M", 20), ("D", 2), ("M", query_len_of(c) - 20)]), False))
    c = _long_cigar(rng)
    L.append(("field_k_not_lseq", dict(cigar=c, aux=_cg(c), cigar_field=[("S", query_len_of(c) - 1), ("N", ref_len_of(c))]), False))
    c = _long_cigar(rng)
    L.append(("field_s_d", dict(cigar=c, aux=_cg(c), cigar_field=[("S", query_len_of(c)), ("D", ref_len_of(c))]), False))
    # ---- a CG tag that is taken and does not fit the sequence: the record is skipped (the documented deviation)
    c = _long_cigar(rng)
    L.append(("cg_wrong_qlen", dict(cigar=c, aux=_cg(c), l_seq=query_len_of(c) + 2,
                                    cigar_field=[("S", query_len_of(c) + 2), ("N", ref_len_of(c))]), True))
    return L


@functools.lru_cache(maxsize=None)
def aux_case():
    """one contig; every layout's read 200 bases behind the one before, an ordinary read (the writer's fixed fields, every other one
    with its CIGAR in the CG tag) between; loci on every base of every read and to either side"""
    rng = np.random.default_rng(20261018)
    reads, layouts, loci = [], [], set()
    for k, (name, extra, taken) in enumerate(_aux_layouts(rng)):
        extra = dict(extra)
        r = _read(rng, name, 0, AUX_FIRST + AUX_STEP * k, extra.pop("cigar"), flag=16 * (k & 1), **extra)
        layouts.append((name, r, taken))
        reads.append(r)
        reads.append(_read(rng, "plain%d" % k, 0, r["pos"] + 110, _long_cigar(rng), cg_tag=bool(k & 1)))
    for r in reads:
        eff = effective_cigar(r)
        span = max(ref_len_of(eff), ref_len_of(r["cigar"]), ref_len_of(r.get("cigar_field", [])))
        loci.update(range(r["pos"], r["pos"] + span + 6))        # 1-based: one base in front of the read .. a few behind it
    length = reads[-1]["pos"] + 400
    assert length < 16384
    ref_seq = _seq(rng, length)
    bam = os.path.join(_dir(), "aux.bam")
    write_bam(bam, [(AUX_CTG, length)], reads, block_payload=1500)
    return dict(bam=bam, reads=reads, layouts=layouts, loci=sorted(loci), ref_seq=ref_seq, length=length)


@functools.lru_cache(maxsize=None)
def aux_expected(params):
    c = aux_case()
    return naive(c["reads"], 0, c["loci"], *AUX_PARAMS[params]), naive_entered(c["reads"], 0, c["loci"], *AUX_PARAMS[params])


def aux_region(read):
    """the 200 bases (1-based, inclusive) that hold one layout's read and the ordinary read behind it"""
    return read["pos"] - 19, read["pos"] + 180


# ------------------------------------------------------------------------------------------------ CRC-32 slice seams
SEAM_SIZES = [1, 1023, 1024, 1025, 2047, 2048, 2049, 64512, 64513, 65280, 65535, 65536]
STORED_SIZE = 65505                                   # the most a stored DEFLATE block leaves room for in a BGZF block
STORED_FLIPS = {"slice0_last": 992, "slice1_first": 993, "slice31": 993 + 1024 * 30 + 500, "slice63_first": 993 + 1024 * 62,
                "block_last": STORED_SIZE - 1}


def _long_reads(rng, n, ref, length, prefix):
    """reads of 600 bases whose records compress well (few distinct qualities): about 1 kB each"""
    reads = []
    for i, pos in enumerate(np.sort(rng.integers(0, length - 700, size=n)).tolist()):
        cigar = [("M", 300), ("I", 2), ("M", 200), ("D", 3), ("M", 98)]
        qual = [10 if k % 7 == 0 else 30 for k in range(600)]
        reads.append(dict(name="%s%04d" % (prefix, i), flag=16 * (i & 1), ref=ref, pos=pos, mapq=60, cigar=cigar, seq=_seq(rng, 600), qual=qual))
    return reads


@functools.lru_cache(maxsize=None)
def seams_case():
    """ordinary reads in blocks of SEAM_SIZES inflated bytes, then ordinary blocks: one slice, one short of two, exactly two, one
    more; the same around 2048; 63 slices, 63 and a byte; the largest blocks the format has.  The BAM header has a block of its own in
    front, so that the one-byte block holds the first byte of the first record and lies in the byte range the index gives for the
    contig (seam_blocks = the file offsets that range has to hold)."""
    rng = np.random.default_rng(1024)
    length = 20000
    reads = _long_reads(rng, 420, 0, length, "s")
    bam = os.path.join(_dir(), "seams.bam")
    header = 12 + 4 + len("seams") + 1 + 4
    sizes = [header] + SEAM_SIZES + [3000] * 100
    info = write_bam(bam, [("seams", length)], reads, block_payload=sizes)
    n = len(SEAM_SIZES)
    assert info["block_sizes"][:n + 1] == [header] + SEAM_SIZES and n + 10 < len(info["block_sizes"]) <= len(sizes)
    assert info["record_spans"][0][0] == header
    loci = list(range(5, length, 37))
    return dict(bam=bam, reads=reads, loci=loci, ref_seq=_seq(rng, length), length=length, want=naive(reads, 0, loci, *PARAMS["verdict"]),
                seam_blocks=(info["block_offsets"][1], info["block_offsets"][n + 1]), n_data_blocks=len(info["block_sizes"]) - 1)


def chunk_span(bam, ctg, loci):
    """[file_begin, file_end) of the bytes the device inflates for the loci (cto_bam_chunk_span)"""
    import ctypes as C
    from clairs_to_amd._lib import check, lib
    fb, fe = C.c_int64(), C.c_int64()
    check(lib.cto_bam_chunk_span(bam.encode(), None, ctg.encode(), loci[0], loci[-1], C.byref(fb), C.byref(fe)))
    return fb.value, fe.value


@functools.lru_cache(maxsize=None)
def stored_case():
    """Stored DEFLATE blocks (level 0: a flipped data byte is a flipped inflated byte, inflate cannot object).  Block 0 ends with the
    last record of contig c0, block 1 - STORED_SIZE bytes, 64 slices, the first of 993 bytes - holds records of c1 only and still
    lies inside the byte range the index gives for c0.  copies: name -> path of a copy with one byte of block 1 damaged."""
    rng = np.random.default_rng(65505)
    refs = [("c0", 3000), ("c1", 30000)]
    reads = [_read(rng, "a%02d" % i, 0, 40 + 60 * i, _long_cigar(rng)) for i in range(40)] + _long_reads(rng, 90, 1, 30000, "b")
    header = 12 + sum(4 + len(n) + 1 + 4 for n, _ in refs)
    first = header + sum(len(_record(r, 0)) for r in reads if r["ref"] == 0)
    bam = os.path.join(_dir(), "stored.bam")
    info = write_bam(bam, refs, reads, block_payload=[first, STORED_SIZE] + [3000] * 40, level=0)
    assert info["block_sizes"][:2] == [first, STORED_SIZE] and info["record_spans"][39][1] == first
    off = info["block_offsets"][1]
    assert info["block_offsets"][2] - off == 65536
    raw = open(bam, "rb").read()
    assert raw[off + 18:off + 23] == struct.pack("<BHH", 1, STORED_SIZE, STORED_SIZE ^ 0xffff)
    data = raw[off + 23:off + 23 + STORED_SIZE]
    flips = {k: (off + 23 + i, 0x5a) for k, i in STORED_FLIPS.items()}
    flips["trailer_crc"] = (off + 23 + STORED_SIZE + 1, 0x10)
    copies = {}
    for name, (at, x) in flips.items():
        b = bytearray(raw)
        b[at] ^= x
        # inflate has nothing to say about the copy: only the CRC-32 can object
        out = zlib.decompressobj(-15).decompress(bytes(b[off + 18:off + 23 + STORED_SIZE]))
        if name == "trailer_crc":
            assert out == data
        else:
            want = bytearray(data)
            want[STORED_FLIPS[name]] ^= x
            assert out == bytes(want)
        assert zlib.crc32(out) & 0xffffffff != struct.unpack_from("<I", b, off + 23 + STORED_SIZE)[0]
        copies[name] = os.path.join(_dir(), "stored_%s.bam" % name)
        open(copies[name], "wb").write(bytes(b))
        open(copies[name] + ".bai", "wb").write(open(bam + ".bai", "rb").read())
    loci = list(range(30, 2900, 3))
    return dict(bam=bam, copies=copies, reads=reads, loci=loci, ref_seq=_seq(rng, 3000), block1=(off, info["block_offsets"][2]),
                want=naive(reads, 0, loci, *PARAMS["verdict"]), entered=naive_entered(reads, 0, loci, *PARAMS["verdict"]))


# ------------------------------------------------------------------------------------------------ fixed fields, the chain
FIELD_REFS = [("f0", 3000), ("f1", 3000), ("f2", 3000)]
FIELD_LOCI = list(range(1000, 1201))                  # on f1, 1-based: the region's first locus 1000, its last 1200
# region name -> (reference index, loci): the region the edge reads are placed around, the contig's first bases (where a record with
# pos = -1 would count if it were let in), the whole last contig (its scan runs into the unplaced records)
FIELD_REGIONS = {"f1": (1, FIELD_LOCI), "f1_head": (1, list(range(1, 41))), "f2": (2, list(range(1, 3001, 2)))}
FIELD_BLOCK = 1700


@functools.lru_cache(maxsize=None)
def fields_case():
    rng = np.random.default_rng(4)
    m = lambda n: [("M", n)]
    reads = [_read(rng, "p%02d" % i, 0, 100 + 90 * i, _long_cigar(rng)) for i in range(30)]
    mid = [
        _read(rng, "pos_minus_one", 1, -1, m(30)),                                # placed on the contig, no position: never enters
        _read(rng, "head", 1, 5, m(30)),
        _read(rng, "ends_before_first", 1, 959, m(40)),                           # last base = 1-based 999
        _read(rng, "ends_on_first", 1, 960, m(40)),                               # last base = locus 1000
        _read(rng, "l_seq_1", 1, 1010, m(1)), _read(rng, "l_seq_2", 1, 1010, m(2)), _read(rng, "l_seq_3", 1, 1010, m(3)),
        _read(rng, "l_seq_0", 1, 1020, m(10), l_seq=0),                           # SEQ `*` with a CIGAR
        _read(rng, "l_seq_0_del", 1, 1021, [("D", 5)], l_seq=0),                  # ... with one that asks for no base: not entered either
        _read(rng, "no_cigar", 1, 1025, [], l_seq=12),
        _read(rng, "", 1, 1030, m(30)),                                           # l_read_name = 1
        _read(rng, "n" * 254, 1, 1040, _long_cigar(rng)),                         # l_read_name = 255
        _read(rng, "mapq_255", 1, 1050, _long_cigar(rng), mapq=255),
        _read(rng, "starts_on_last", 1, 1199, m(40)),                             # first base = locus 1200
        _read(rng, "starts_behind_last", 1, 1200, m(40)),
    ]
    mid += [_read(rng, "m%02d" % i, 1, 300 + 55 * i, _long_cigar(rng), flag=16 * (i & 1)) for i in range(40)]
    mid.sort(key=lambda r: r["pos"])
    last = [_read(rng, "q%02d" % i, 2, 10 + 90 * i, _long_cigar(rng)) for i in range(30)]
    tail = [_read(rng, "u%02d" % i, -1, -1, [], flag=4, mapq=0, l_seq=50) for i in range(12)]
    reads = reads + mid + last + tail
    bam = os.path.join(_dir(), "fields.bam")
    info = write_bam(bam, FIELD_REFS, reads, block_payload=FIELD_BLOCK)
    # reads of the contig in front share the first block of f1's records, reads of the one behind share the last
    spans = info["record_spans"]
    first_mid, first_last = spans[30][0], spans[30 + len(mid)][0]
    assert first_mid % FIELD_BLOCK > 200 and first_last % FIELD_BLOCK > 200
    return dict(bam=bam, reads=reads)


@functools.lru_cache(maxsize=None)
def fields_expected(region, params):
    ri, loci = FIELD_REGIONS[region]
    reads = fields_case()["reads"]
    return naive(reads, ri, loci, *AUX_PARAMS[params]), naive_entered(reads, ri, loci, *AUX_PARAMS[params])


LYING = ("fields_past_block_size", "end_past_int32", "block_size_20")


@functools.lru_cache(maxsize=None)
def lying_case(kind):
    """good reads and, among them, one record whose fields lie; the index files it as an ordinary 20M read"""
    rng = np.random.default_rng(LYING.index(kind))
    reads = [_read(rng, "g%02d" % i, 0, 50 + 40 * i, _long_cigar(rng)) for i in range(40)]
    honest = _read(rng, "liar", 0, 805, [("M", 20)])
    if kind == "fields_past_block_size":
        raw = bytearray(_record(honest, 0))
        struct.pack_into("<H", raw, 4 + 12, 60000)                                # n_cigar_op: 240 000 bytes of CIGAR in a 100-byte record
    elif kind == "end_past_int32":
        far = [("M", 10)] + [("D", (1 << 28) - 1)] * 8 + [("M", 10)]              # 805 + 20 + 8 * (2^28 - 1) > 2^31 - 1
        assert 805 + ref_len_of(far) > 2 ** 31 - 1
        raw = _record(dict(honest, cigar=far, aux=b""), 0)
    else:
        raw = struct.pack("<i", 20) + bytes(_record(honest, 0)[4:24])            # a record of 20 bytes: not even the fixed fields
    k = next(i for i, r in enumerate(reads) if r["pos"] > honest["pos"])
    reads.insert(k, dict(honest, raw=bytes(raw)))
    bam = os.path.join(_dir(), kind + ".bam")
    write_bam(bam, [("liar", 3000)], reads, block_payload=1500)
    return dict(bam=bam, loci=list(range(1, 2000, 3)), ref_seq=_seq(rng, 3000))
