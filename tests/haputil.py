"""Test-only: the haplotype-filter fixtures as BAM files, and a haplotype-filter job (csrc/hapfilter.cpp) as plain Python values.

reads_of turns a tests/golden/hapsim.py simulation into bamutil.write_bam reads that pile up to the rows hapsim.pileup_rows prints;
job_columns turns a job's view into lists that compare with ==; stage_args is the Namespace of the haplotype_filtering stage."""
import os
import struct
import sys
from argparse import Namespace

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, "golden") not in sys.path:
    sys.path.insert(0, os.path.join(HERE, "golden"))


def reads_of(sim, ref_index=0):
    """pos = s; CIGAR from the edits inside [s, e): M runs, I, D of min(len, e - p - 1), edits inside a deleted span dropped as
    pileup_rows drops them; SEQ = the reference with the substitutions; QUAL 30 or the read's bq[p]; MAPQ mq; flag 16 when rev; HP of
    an integer type when tagged."""
    ref, out, names = sim["ref"], [], set()
    for n_read, r in enumerate(sim["reads"]):
        s, e = r["s"], r["e"]
        cigar, seq, qual = [], [], []

        def op(kind, n):
            if cigar and cigar[-1][0] == kind:
                cigar[-1] = (kind, cigar[-1][1] + n)
            else:
                cigar.append((kind, n))
        p = s
        while p < e:
            ed = r["edits"].get(p)
            seq.append(ed[1] if ed is not None and ed[0] == "X" else ref[p])
            qual.append(r["bq"].get(p, 30))
            op("M", 1)
            if ed is not None and ed[0] == "I":
                op("I", len(ed[1]))
                seq.extend(ed[1])
                qual.extend([30] * len(ed[1]))
            elif ed is not None and ed[0] == "D":
                n = min(ed[1], e - p - 1)
                if n > 0:
                    op("D", n)
                    p += n
            p += 1
        assert cigar[0][0] == "M" and cigar[-1][0] == "M", "read %s starts or ends in an indel: %r" % (r["name"], cigar[:2] + cigar[-2:])
        assert r["name"] not in names, "read name %s repeats" % r["name"]
        names.add(r["name"])
        # the six integer types in turn: every one is an HP value
        ty = "cCsSiI"[n_read % 6]
        aux = (b"HP" + ty.encode() + struct.pack("<" + {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I"}[ty], r["hap"])) if r["tagged"] else b""
        out.append(dict(name=r["name"], flag=16 if r["rev"] else 0, ref=ref_index, pos=s, mapq=r["mq"], cigar=cigar, seq="".join(seq),
                        qual=qual, aux=b"NMi" + struct.pack("<i", 1) + aux))
    return out


def job_columns(view, bq_of_placeholders=True):
    """[(pos, [(key, base, indel, bq, mq, hp, hp_single)], [start / end indices])], columns without a record left out (no rule tells
    them from absent ones); bq_of_placeholders=False blanks the BQ of `*` / `#` records"""
    out = []
    recs, keys, indels = view["recs"], view["keys"], view["indels"]
    for c in range(len(view["col_pos"])):
        a, b = int(view["col_off"][c]), int(view["col_off"][c + 1])
        if a == b:
            continue
        rows = []
        for r in recs[a:b]:
            base = chr(r["base"])
            ind = indels[int(r["indel_off"]):int(r["indel_off"]) + int(r["indel_len"])] if r["indel_len"] else b""
            bq = int(r["bq"]) if bq_of_placeholders or base not in "*#" else None
            rows.append((keys[int(r["read"])], base, ind, bq, int(r["mq"]), chr(r["hp"]), int(r["hp_single"])))
        out.append((int(view["col_pos"][c]), rows, [int(x) for x in view["rse"][int(view["rse_off"][c]):int(view["rse_off"][c + 1])]]))
    return out


def first_difference(a, b):
    """for an assertion message: the first column in which two job_columns lists differ"""
    for x, y in zip(a, b):
        if x != y:
            if x[0] != y[0]:
                return "columns %d / %d" % (x[0], y[0])
            for i, (u, v) in enumerate(zip(x[1], y[1])):
                if u != v:
                    return "column %d record %d: %r / %r" % (x[0], i, u, v)
            return "column %d: %d / %d records, start-end %r / %r" % (x[0], len(x[1]), len(y[1]), x[2], y[2])
    return "%d / %d columns" % (len(a), len(b))


def rows_positions(text):
    return sorted({int(row.split("\t")[1]) for row in text.split("\n") if row})


def merged_intervals(positions):
    """sorted 1-based positions -> merged 0-based [s, e)"""
    out = []
    for p in positions:
        if out and out[-1][1] == p - 1:
            out[-1][1] = p
        else:
            out.append([p - 1, p])
    return out


def write_inputs(d, ctg, ref, germline_vcf, pileup_vcf):
    (d / "ref.fa").write_text(">%s\n%s\n" % (ctg, ref))
    (d / "ref.fa.fai").write_text("%s\t%d\t%d\t%d\t%d\n" % (ctg, len(ref), len(ctg) + 2, len(ref), len(ref) + 1))
    (d / "germline.vcf").write_text(germline_vcf)
    (d / "pileup.vcf").write_text(pileup_vcf)


def wide_inputs(sim, ctg):
    """{mode: pileup VCF text} of a contig of tests/golden/hapfilter_wide.json.gz: gen_hapfilter_wide.inputs_for's VCF, which reads
    only the rows at the calls themselves - so without the flanks, whose text nobody wants here (tests/test_haplotype_filtering.py
    holds the simulator to the fixture's digest; a drift would show in the output VCF here too)"""
    import gen_hapfilter_wide as gw
    return {mode: gw.inputs_for(sim, ctg, mode, flank=0)[0] for mode in ("snv", "indel")}


def stage_args(d, ctg, bam, mode, out_name, where, **over):
    a = Namespace(tumor_bam_fn=str(bam), ref_fn=str(d / "ref.fa"), ctg_name=ctg, pileup_vcf_fn=str(d / "pileup.vcf"),
                  output_vcf_fn=str(d / out_name), germline_vcf_fn=str(d / "germline.vcf"), output_dir=str(d / ("work_" + out_name)), threads=4,
                  input_filter_tag=None, show_ref=False, samtools="samtools", mpileup_fn=None, pileup_source="bam", where=where,
                  reverse_del=True, apply_haplotype_filtering=True, min_mq=20, min_bq=0, min_alt_coverage=2, is_indel=(mode == "indel"),
                  test_pos=None, flanking=100, haplotype_chunk_max_sites=200, haplotype_chunk_max_span=5000000,
                  haplotype_chunk_mpileup_bed=True, disable_read_start_end_filtering=False)
    for k, v in over.items():
        setattr(a, k, v)
    return a


# ------------------------------------------------------------------------------------------ a BAM written out by hand
HAND_CTG, HAND_LEN = "c1", 400
HAND_WANTED = [1, 5, 11, 12, 16, 17, 18, 19, 20, 23, 30, 31, 101, 111, 133, 327, 328, 329, 360]      # 1-based


def hand_reads():
    """A dozen kept reads and six excluded ones over one 400-base contig; each is the smallest shape of one thing that can go wrong
    (see hand_covers for what they print)."""
    def rd(name, pos, cigar, seq, qual, flag=0, mapq=60, **kw):
        return dict(name=name, flag=flag, ref=0, pos=pos, mapq=mapq, cigar=cigar, seq=seq, qual=qual, **kw)
    c20 = "C" * 20
    reads = [
        rd("z", 0, [("M", 5)], "GATTA", [30] * 5, aux=b""),                               # the window clipped at position 1
        rd("x4", 10, [("M", 20)], c20, [30] * 20, flag=4, aux=b""),                       # each bit of 2316 ...
        rd("x8", 10, [("M", 20)], c20, [30] * 20, flag=1 | 2 | 8, aux=b""),
        rd("x256", 10, [("M", 20)], c20, [30] * 20, flag=256, aux=b""),
        rd("x2048", 10, [("M", 20)], c20, [30] * 20, flag=2048, aux=b""),
        rd("orphan", 10, [("M", 20)], c20, [30] * 20, flag=1, aux=b""),                   # ... an orphan ...
        rd("lowmq", 10, [("M", 20)], c20, [30] * 20, mapq=19, aux=b""),                   # ... MAPQ one below min_mq
        rd("a", 10, [("M", 20)], "ACGTACGTACGTACGTACGT", [5] + [30] * 18 + [5], aux=b"HPC\x01"),      # head and tail base below min_bq 10
        rd("b", 11, [("M", 20)], "=R" + "GT" * 9, None, flag=16, mapq=50, aux=b"HPi" + struct.pack("<i", 12)),   # = and IUPAC, no QUAL, HP 12
        rd("d", 12, [("M", 10)], "T" * 10, [20] * 10, mapq=40, aux=b"HPZ1\0"),            # HP:Z is no HP; the same qname twice on a strand
        rd("d", 13, [("M", 10)], "G" * 10, [21] * 10, mapq=41, aux=b""),
        rd("n", 14, [("M", 2), ("N", 3), ("M", 2)], "CCAA", [31, 32, 33, 34], aux=b"HPC\x02"),       # a skip over wanted columns
        rd("e", 15, [("M", 3), ("D", 2), ("M", 3)], "ACGTTT", [22, 23, 24, 25, 26, 27], flag=16, mapq=33, aux=b"HPs" + struct.pack("<h", 2)),
        rd("g", 16, [("M", 4)], "TTTT", [28] * 4, cg_tag=True),                           # the CIGAR lives in CG:B,I
        rd("k65", 100, [("M", 1), ("I", 1)] * 32 + [("M", 1)], "AC" * 32 + "A", [30] * 65, aux=b"HPS" + struct.pack("<H", 1)),   # 65 operations
        rd("k129", 200, [("M", 1), ("D", 1)] * 64 + [("M", 1)], "G" * 65, [30] * 65, flag=16, aux=b""),     # 129 operations
    ]
    reads += [rd("m%d" % i, 349 + i, [("M", 20)], "A" * 20, [30] * 20, aux=b"") for i in range(1, 7)]      # six covers of column 360
    return reads


def hand_covers(reverse_del):
    """What the reads above print, column by column and cover by cover, written out by hand: (token, BQ, MQ, name, HP field).  `>` is
    the skip of read n: a cover without a base, so the bases behind it pair with the names one place ahead."""
    D = "#" if reverse_del else "*"
    a = lambda tok, bq=30: (tok, bq, 60, "a", "1")
    b = lambda tok: (tok, 0, 50, "b", "12")
    d1, d2 = ("T", 20, 40, "d", "*"), ("G", 21, 41, "d", "*")
    n = lambda tok, bq: (tok, bq, 60, "n", "2")
    e = lambda tok, bq: (tok, bq, 33, "e", "2")
    g = lambda tok: (tok, 28, 60, "g", "*")
    m = lambda i: ("A", 30, 60, "m%d" % i, "*")
    return {
        1: [("^]G", 30, 60, "z", "*")],
        5: [("A$", 30, 60, "z", "*")],
        11: [a("^]A", 5)],
        12: [a("C"), b("^Sn")],
        16: [a("C"), b("g"), d1, d2, n("C", 32), e("^Ba", 22)],
        17: [a("G"), b("t"), d1, d2, n(">", 33), e("c", 23), g("^]T")],
        18: [a("T"), b("g"), d1, d2, n(">", 33), e("g-2nn", 24), g("T")],
        19: [a("A"), b("t"), d1, d2, n(">", 33), e(D, 25), g("T")],
        20: [a("C"), b("g"), d1, d2, n("A", 33), e(D, 25), g("T$")],
        23: [a("A"), b("t"), ("G$", 21, 41, "d", "*"), e("t$", 27)],
        30: [a("T$", 5), b("g")],
        31: [b("t$")],
        101: [("^]A+1C", 30, 60, "k65", "1")],
        111: [("A+1C", 30, 60, "k65", "1")],
        133: [("A$", 30, 60, "k65", "1")],
        327: [("g-1n", 30, 60, "k129", "*")],
        328: [(D, 30, 60, "k129", "*")],
        329: [("g$", 30, 60, "k129", "*")],
        360: [m(i) for i in range(1, 7)],
    }


def hand_rows(covers, min_bq=0, keep=None):
    """the nine-column text of hand-written covers; a cover below min_bq prints nothing.  keep: only these read names (the depth cap)"""
    rows = []
    for pos in sorted(covers):
        t = [c for c in covers[pos] if c[1] >= min_bq and (keep is None or c[3] in keep)]
        if t:
            rows.append("%s\t%d\tN\t%d\t%s\t%s\t%s\t%s\t%s\n" % (HAND_CTG, pos, len(t), "".join(c[0] for c in t), "".join(chr(c[1] + 33) for c in t),
                                                                  "".join(chr(c[2] + 33) for c in t), ",".join(c[3] for c in t), ",".join(c[4] for c in t)))
    return "".join(rows)
