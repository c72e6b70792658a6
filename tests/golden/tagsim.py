"""Synthetic inputs of the Verdict step tag_germline_variant (src/verdict/tag_germline_variant.py of the reference): a VCF of calls, the
purity / ploidy file and the copy-number table that run_ascat would write.  Input synthesis for gen_tag_germline.py and for the tests,
which regenerate the inputs from the specs and check them against the stored SHA-256.  The product never imports this.

files(spec): spec = dict(seed, purity, contigs=[(name, length)], segments=[(contig, start, end, nMajor, nMinor, quoted)] in file order,
rows, targeted=[(segment number, depth, AF text)], deep, edges, gz, omit=[file names]).  `rows` random calls: a contig, a position anywhere on it
(so some lie in no segment, and a contig without a segment has only such calls), a depth of 8 - 300 (`deep` of them 1000 - 3000), a FILTER
(PASS four times out of five), a FORMAT with AF or VAF.  The AF of a call inside a segment is, six times out of ten, what a draw of its
reads from one of the segment's expected fractions or from halfway between two of them gives, so that every branch of the decision
tree is near; otherwise it is uniform on [0, 1].  It is written with four decimals, so the text is the number.  Then: the targeted calls,
one call on the start and one on the end of every segment (when `edges` is set), a non-PASS row that ends in blanks, a PASS row that ends in blanks, and one
row that repeats the contig and position of an earlier one.  Rows are sorted by contig and position, the repeat put last.
The VCF is `in.vcf`, or `in.vcf.gz` (gzip, no time stamp) when gz is set; the others are `purity.txt` and `cna.txt`."""
import gzip
import hashlib
import io
import random

HEADER = ("##fileformat=VCFv4.2\n##FILTER=<ID=PASS,Description=\"All filters passed\">\n##FILTER=<ID=LowQual,Description=\"Low quality variant\">\n"
          "##INFO=<ID=H,Number=0,Type=Flag,Description=\"Variant found only in one haplotype in the phased reads\">\n%s"
          "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n##FORMAT=<ID=DP,Number=1,Type=Integer,Description=\"Read Depth\">\n"
          "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n")


def digest(files):
    h = hashlib.sha256()
    for k in sorted(files):
        h.update(k.encode())
        h.update(gzip.decompress(files[k]) if isinstance(files[k], bytes) else files[k].encode())       # what is in it, not how it was packed
    return h.hexdigest()


def expected_fractions(p, major, minor):
    M, C = minor, major + minor
    if M == 0:
        M = C
    den = p * C + 2 * (1 - p)
    out = [(p * M + 1 - p) / den, p * M / den]
    if M != C - M:
        out.append((p * (C - M) + 1 - p) / den)
        if C - M:
            out.append(p * (C - M) / den)
    return out


def row_text(rng, ctg, pos, depth, af, flt, tail=""):
    ref = rng.choice("ACGT")
    alt = rng.choice([b for b in "ACGT" if b != ref])
    if rng.random() < 0.15:
        ref += "".join(rng.choice("ACGT") for _ in range(rng.randint(1, 4)))
    tag = "VAF" if rng.random() < 0.2 else "AF"
    fmt, val = "GT:GQ:DP:" + tag, "0/1:%d:%d:%s" % (rng.randint(2, 40), depth, af)
    if rng.random() < 0.5:
        alt_reads = int(round(depth * float(af)))
        fmt, val = fmt + ":AD", val + ":%d,%d" % (depth - alt_reads, alt_reads)
    info = rng.choice(["H", ".", "FAU=%d;FCU=%d" % (rng.randint(0, 9), rng.randint(0, 9))])
    return "%s\t%d\t.\t%s\t%s\t%.4f\t%s\t%s\t%s\t%s%s\n" % (ctg, pos, ref, alt, rng.uniform(2, 40), flt, info, fmt, val, tail)


def files(spec):
    rng = random.Random(spec["seed"])
    p, segments = spec["purity"], spec["segments"]
    lengths = dict(spec["contigs"])
    rows, used = [], set()

    def free(ctg, lo, hi):
        for _ in range(1000):
            pos = rng.randint(lo, hi)
            if (ctg, pos) not in used and all(pos not in (s[1], s[2]) for s in segments if s[0] == ctg):
                used.add((ctg, pos))
                return pos
        raise AssertionError("no free position")

    def first_segment(ctg, pos):
        for s in segments:
            if s[0] == ctg and s[1] <= pos <= s[2]:
                return s
        return None

    def drawn_af(seg, depth):
        if seg is None or rng.random() >= 0.6:
            return "%.4f" % rng.random()
        e = expected_fractions(p, seg[3], seg[4])
        centre = rng.choice(e) if rng.random() < 0.6 else (rng.choice(e) + rng.choice(e)) / 2
        k = sum(rng.random() < centre for _ in range(depth))
        return "%.4f" % min(1.0, max(0.0001, k / depth + rng.uniform(-0.4, 0.4) / depth))

    for i in range(spec["rows"]):
        ctg = rng.choice(spec["contigs"])[0]
        pos = free(ctg, 1, lengths[ctg])
        depth = rng.randint(1000, 3000) if i < spec["deep"] else int(round(8 * (300 / 8) ** rng.random()))
        flt = "PASS" if rng.random() < 0.8 else rng.choice(["LowQual", "NonSomatic", "LowQual;NonSomatic"])
        rows.append((ctg, pos, row_text(rng, ctg, pos, depth, drawn_af(first_segment(ctg, pos), depth), flt)))
    for number, depth, af in spec["targeted"]:
        s = segments[number]
        for _ in range(1000):
            pos = free(s[0], s[1] + 1, s[2] - 1)
            if first_segment(s[0], pos) is s:
                break
        rows.append((s[0], pos, row_text(rng, s[0], pos, depth, af, "PASS")))
    for s in segments if spec["edges"] else []:
        for pos in (s[1], s[2]):
            if (s[0], pos) not in used:
                used.add((s[0], pos))
                depth = rng.randint(20, 200)
                rows.append((s[0], pos, row_text(rng, s[0], pos, depth, drawn_af(first_segment(s[0], pos), depth), "PASS")))
    if spec["rows"]:
        ctg = spec["contigs"][0][0]
        pos = free(ctg, 1, lengths[ctg])
        rows.append((ctg, pos, row_text(rng, ctg, pos, 40, "0.3000", "LowQual", tail="  \t ")))
        s = segments[0]
        pos = free(s[0], s[1] + 1, s[2] - 1)
        rows.append((s[0], pos, row_text(rng, s[0], pos, 60, "0.4500", "PASS", tail=" \t")))
    order = {c[0]: i for i, c in enumerate(spec["contigs"])}
    rows.sort(key=lambda r: (order[r[0]], r[1]))
    if spec["rows"]:
        again = [r for r in rows if "PASS" in r[2] and first_segment(r[0], r[1]) is not None][3]
        rows.append((again[0], again[1], row_text(rng, again[0], again[1], 90, "0.9700", "PASS")))
    vcf = HEADER % "".join("##contig=<ID=%s,length=%d>\n" % tuple(c) for c in spec["contigs"]) + "".join(r[2] for r in rows)
    cna = "Sample\tChromosome\tStartPosition\tEndPosition\tnMajor\tnMinor\n" + "".join(
        "TUM\t%s\t%d\t%d\t%d\t%d\n" % ('"%s"' % s[0] if s[5] else s[0], s[1], s[2], s[3], s[4]) for s in segments)
    out = {"purity.txt": "Sample\tPurity\tPloidy\tGoodnessOfFit\nTUM\t%s\t2.31\t97.5\n" % p, "cna.txt": cna}
    if spec["gz"]:
        buf = io.BytesIO()
        with gzip.GzipFile(fileobj=buf, mode="wb", mtime=0) as g:
            g.write(vcf.encode())
        out["in.vcf.gz"] = buf.getvalue()
    else:
        out["in.vcf"] = vcf
    for name in spec["omit"]:
        del out[name]
    return out


def write(d, built):
    import os
    for k, v in built.items():
        with open(os.path.join(d, k), "wb" if isinstance(v, bytes) else "w") as f:
            f.write(v)
