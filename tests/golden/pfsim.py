"""Synthetic short-read pileups for the postfilter fixtures: what
`samtools mpileup --min-MQ q --min-BQ q --excl-flags 2316 -r <region> --output-MQ --output-QNAME` prints for an Illumina-like tumour BAM -
eight columns: chr, pos, ref, depth, bases (with ^<mq> read starts and $ read ends), BQ, MQ, read names - on small contigs seeded with a
catalogue of calls designed to trip each filter of src/postfilter_variants.py (ReadStartEnd, VariantCluster, StrandBias, LowSeqEntropy),
several at once, and none; and the odd inputs of the issue (repeated read keys in a column, a row that opens with '^', shallow columns,
calls next to the contig start, calls with no alt read, positions without a row, insertions longer than 2 x flanking, deletions whose
length does and does not match REF, '*' / '#' entries).  Input synthesis for gen_postfilter.py and the tests that regenerate its inputs
from the seeds; the product never imports this."""
import hashlib
import random

ACGT = "ACGT"
HEAD = ("##fileformat=VCFv4.2\n##source=ClairS-TO\n##FILTER=<ID=PASS,Description=\"All filters passed\">\n"
        "##FILTER=<ID=LowQual,Description=\"Low-quality variant\">\n##FILTER=<ID=RefCall,Description=\"Reference call\">\n"
        "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n##FORMAT=<ID=AF,Number=1,Type=Float,Description=\"AF\">\n"
        "##FORMAT=<ID=TU,Number=1,Type=Integer,Description=\"Count of T in the tumor BAM\">\n"
        "##contig=<ID=dropped,length=1>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n")


def other(b, k=1):
    return ACGT[(ACGT.index(b) + k) % 4]


def simulate(seed, length=5200, depth=40, read_len=150, odd=False):
    """-> dict(ref, reads, snv_calls [(pos1, ref, alt)], indel_calls)"""
    rng = random.Random(seed)
    ref = [rng.choice(ACGT) for _ in range(length)]
    for lo in (2000, 3600):                                    # low-complexity stretches for the sequence-entropy filter
        for i in range(lo, lo + 60):
            ref[i] = "A" if i < lo + 30 else "AC"[i & 1]
    ref = "".join(ref)
    reads = []
    for i in range(depth * length // read_len):
        s = rng.randint(-read_len + 20, length - 20)
        e = min(length, s + read_len + rng.randint(-10, 10))
        s = max(0, s)
        if e - s >= 30:
            reads.append(dict(name="q%d.%d" % (seed, i), s=s, e=e, rev=rng.random() < 0.5, edits={}))
    if odd:
        gap = 1500                                             # no coverage over [gap, gap + 25), then six reads starting together
        reads = [r for r in reads if r["e"] <= gap or r["s"] >= gap + 25]
        for i in range(6):
            reads.append(dict(name="g%d.%d" % (seed, i), s=gap + 25, e=gap + 25 + read_len, rev=i % 2 == 1, edits={}))
        for i in range(0, 40, 2):                              # repeated keys: two records of one name on one strand
            a, b = reads[i * 7], reads[i * 7 + 1]
            b["name"], b["rev"] = a["name"], a["rev"]
    reads.sort(key=lambda r: r["s"])

    def covering(p, margin=1):
        return [r for r in reads if r["s"] + margin <= p < r["e"] - margin]
    snv, indel = [], []
    taken = set()

    def site(lo=130, hi=None):
        hi = hi or length - 130
        while True:
            q = rng.randint(lo, hi)
            if all(abs(q - t) > 9 for t in taken) and not any(l - 8 <= q <= l + 68 for l in (2000, 3600)):
                taken.add(q)
                return q

    def put_snv(q, pick, alt=None):
        ab = alt or other(ref[q], 2)
        for r in covering(q, 0):
            if q not in r["edits"] and pick(r):
                r["edits"][q] = ("X", ab)
        snv.append((q + 1, ref[q], ab))

    def put_indel(q, kind, pick, seq="TG", dl=3, call_dl=None):
        for r in covering(q, dl + 3):
            if q not in r["edits"] and pick(r):
                r["edits"][q] = ("I", seq) if kind == "I" else ("D", dl)
        n = call_dl or dl
        indel.append((q + 1, ref[q], ref[q] + seq) if kind == "I" else (q + 1, ref[q:q + n + 1], ref[q]))

    for k in range(22):                                        # clean calls at a range of allele fractions
        put_snv(site(), lambda r, f=0.1 + 0.03 * k: rng.random() < f)
    for k in range(14):                                        # strand bias of graded strength (p from ~1e-2 down to ~1e-9)
        leak = (0.0, 0.05, 0.1, 0.15, 0.2, 0.25, 0.3)[k % 7]
        put_snv(site(), lambda r, leak=leak: rng.random() < (0.55 if not r["rev"] else 0.55 * leak))
    for k in range(10):                                        # the alt allele sits on reads that end right there
        q = site(400, length - 400)
        near = [r for r in reads if 0 < r["e"] - (q + 1) < 60 and not r["edits"]][:12 + k]
        for r in near:
            r["e"] = q + 1
        ids = {id(r) for r in near}
        put_snv(q, lambda r: id(r) in ids or rng.random() < 0.03)
    for k in range(10):                                        # clusters: the supporting reads share further mismatches nearby
        q = site(300, length - 300)
        sup = [r for r in covering(q, 45) if rng.random() < 0.4 and (k % 3 or not r["rev"])]
        ids = {id(r) for r in sup}
        put_snv(q, lambda r: id(r) in ids)
        for d in ((-21, 17), (-33, 12, 40), (25,))[k % 3]:
            taken.add(q + d)
            for r in sup:
                if q + d not in r["edits"]:
                    r["edits"][q + d] = ("X", other(ref[q + d], 3))
    for k in range(3):                                         # a long insertion next to the call (longer than 2 x flanking on k == 0)
        q = site(300, length - 300)
        put_snv(q, lambda r: rng.random() < 0.3)
        taken.add(q + 15)
        for r in covering(q + 15, 8)[:3 + 2 * k]:
            r["edits"][q + 15] = ("I", "ACGTTGCA" * (32 if k == 0 else 12))
    put_snv(45, lambda r: rng.random() < 0.4)                  # window clipped at position 1
    put_snv(100, lambda r: rng.random() < 0.4)
    q = site()
    snv.append((q + 1, ref[q], other(ref[q], 1)))              # a call no read supports
    put_snv(site(), lambda r: rng.random() < 0.3)
    if odd:
        put_snv(1500 + 25, lambda r: r["name"].startswith("g") and not r["rev"])      # on the row that opens with '^'
        put_snv(1500 + 60, lambda r: rng.random() < 0.5)
        snv.append((1500 + 10, ref[1500 + 9], other(ref[1500 + 9])))                     # a position with no row
        put_snv(1500 - 30, lambda r: rng.random() < 0.5)
    # indel calls
    for k in range(8):
        put_indel(site(), "I" if k % 2 else "D", lambda r, f=0.2 + 0.05 * k: rng.random() < f, seq=("TG", "A", "GGA", "C")[k % 4], dl=1 + k % 3)
    for k in range(5):
        put_indel(site(), "ID"[k % 2], lambda r: (not r["rev"]) and rng.random() < 0.6, dl=2)
    for lo in (2000, 3600):                                    # inside the low-complexity stretches
        put_indel(lo + 10, "D", lambda r: rng.random() < 0.4, dl=2)
        put_indel(lo + 24, "I", lambda r: (not r["rev"]) and rng.random() < 0.5, seq="A")
        put_indel(lo + 44, "I", lambda r: rng.random() < 0.4, seq="AC")
    put_indel(site(), "D", lambda r: rng.random() < 0.4, dl=2, call_dl=3)            # the reads' deletion is shorter than REF says
    put_indel(site(), "I", lambda r: rng.random() < 0.4, seq="ACGTTGCA" * 30)        # an insertion call longer than 2 x flanking
    for k in range(3):
        q = site(400, length - 400)
        near = [r for r in reads if 8 < r["e"] - (q + 1) < 60 and not r["edits"]][:14]
        for r in near:
            r["e"] = q + 6
        ids = {id(r) for r in near}
        put_indel(q, "I", lambda r: id(r) in ids, seq="T")
    for r in reads:                                            # sequencing noise
        for _ in range(max(1, (r["e"] - r["s"]) // 120)):
            q = rng.randint(r["s"], r["e"] - 1)
            if not any(q - 6 <= k2 <= q + 1 for k2 in r["edits"]):
                r["edits"][q] = ("X", other(ref[q], rng.randint(1, 3)))
    reads.sort(key=lambda r: r["s"])
    return dict(ref=ref, reads=reads, snv_calls=sorted(set(snv)), indel_calls=sorted(set(indel)))


def pileup_text(sim, ctg, positions):
    """eight-column rows for the given 1-based positions"""
    ref, want, rows = sim["ref"], set(positions), {}
    for r in sim["reads"]:
        p, hi, skip, first = r["s"], r["e"], 0, True
        while p < hi:
            ed = r["edits"].get(p) if skip == 0 else None
            if skip > 0:
                tok = "#" if r["rev"] else "*"
                skip -= 1
            else:
                b = ed[1] if ed is not None and ed[0] == "X" else ref[p]
                tok = b.lower() if r["rev"] else b
                if ed is not None and ed[0] == "I":
                    tok += "+%d%s" % (len(ed[1]), ed[1].lower() if r["rev"] else ed[1])
                elif ed is not None and ed[0] == "D":
                    n = min(ed[1], hi - p - 1)
                    if n > 0:
                        tok += "-%d%s" % (n, ("n" if r["rev"] else "N") * n)
                        skip = n
            if first:
                tok, first = "^]" + tok, False
            if p == hi - 1:
                tok += "$"
            if p + 1 in want:
                rows.setdefault(p + 1, []).append((tok, r["name"]))
            p += 1
    return "".join("%s\t%d\tN\t%d\t%s\t%s\t%s\t%s\n" % (ctg, p, len(t), "".join(x[0] for x in t), "I" * len(t), "]" * len(t), ",".join(x[1] for x in t))
                   for p, t in sorted(rows.items()))


def vcf_rows(sim, ctg, mode, rows_by_pos):
    calls = sim["snv_calls"] if mode == "snv" else sim["indel_calls"]
    out = []
    for i, (p, rb, ab) in enumerate(calls):
        cols = rows_by_pos.get(p)
        toks = cols[7].count(",") + 1 if cols else 1
        n_alt = (sum(1 for c in cols[4].upper() if c == ab) if len(rb) == 1 and len(ab) == 1 else cols[4].count("+") + cols[4].count("-")) if cols else 0
        af = min(1.0, n_alt / float(toks))
        flt, gt = ("PASS", "0/1") if i % 9 != 8 else (("LowQual", "0/1") if i % 18 == 8 else ("RefCall", "0/0"))
        out.append("%s\t%d\t.\t%s\t%s\t%.4f\t%s\tFAU=1;FCU=2;FGU=3;FTU=4\tGT:GQ:DP:AF:AD:AU:CU:GU:TU\t%s:%d:%d:%.4f:%d,%d:1:2:3:4\n"
                   % (ctg, p, rb, ab, 12.5 + i, flt, gt, 12 + i % 40, toks, af, toks - n_alt, n_alt))
    return out


def scenario_files(spec, flank=100):
    """{file name: text} of a scenario: ref.fa, ref.fa.fai, in_snv.vcf, in_indel.vcf, mp.txt (rows of every contig, both passes' windows).
    spec: dict(contigs=[(name, seed)], odd=bool)"""
    fa, fai, mp, vcf = "", "", "", {"snv": [], "indel": []}
    for ctg, seed in spec["contigs"]:
        sim = simulate(seed, odd=spec.get("odd", False))
        positions = sorted({p for c in sim["snv_calls"] + sim["indel_calls"] for p in range(max(1, c[0] - flank - 1), c[0] + flank + 2)})
        text = pileup_text(sim, ctg, positions)
        by_pos = {int(r.split("\t", 2)[1]): r.rstrip("\n").split("\t") for r in text.split("\n") if r}
        for mode in vcf:
            vcf[mode] += vcf_rows(sim, ctg, mode, by_pos)
        fai += "%s\t%d\t%d\t60\t61\n" % (ctg, len(sim["ref"]), len(fa) + len(ctg) + 2)
        fa += ">%s\n" % ctg + "".join(sim["ref"][i:i + 60] + "\n" for i in range(0, len(sim["ref"]), 60))
        mp += text
    return {"ref.fa": fa, "ref.fa.fai": fai, "mp.txt": mp, "in_snv.vcf": HEAD + "".join(vcf["snv"]), "in_indel.vcf": HEAD + "".join(vcf["indel"])}


def digest(files):
    h = hashlib.sha256()
    for k in sorted(files):
        h.update(k.encode())
        h.update(files[k].encode())
    return h.hexdigest()


# `samtools` for the reference and for the mirror alike: `mpileup ... -r ctg:lo-hi <bam>` serves the rows of ./mp.txt, `faidx <fa> ctg:lo-hi`
# the reference of ./ref.fa (both relative to the working directory of the scenario)
SHIM_SAMTOOLS = r'''#!/usr/bin/env python3
import sys
a = sys.argv[1:]
if a[0] == "faidx":
    ctg, rng = a[2].rsplit(":", 1)
    lo, hi = [int(x) for x in rng.split("-")]
    seq, on = [], False
    for line in open(a[1]):
        if line.startswith(">"):
            on = line[1:].strip() == ctg
        elif on:
            seq.append(line.strip())
    sub = "".join(seq)[lo - 1:hi]
    sys.stdout.write(">%s\n" % a[2])
    for i in range(0, len(sub), 60):
        sys.stdout.write(sub[i:i + 60] + "\n")
elif a[0] == "mpileup":
    ctg, rng = a[a.index("-r") + 1].rsplit(":", 1)
    lo, hi = [int(x) for x in rng.split("-")]
    for row in open("mp.txt"):
        c = row.split("\t", 2)
        if c[0] == ctg and lo <= int(c[1]) <= hi:
            sys.stdout.write(row)
else:
    sys.exit(1)
'''
