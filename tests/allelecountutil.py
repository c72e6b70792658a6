"""Test-only: a deliberately naive restatement of alleleCounter's counting rules (the list at the top of csrc/allelecount.hip) over the
read dicts tests/bamutil.py:write_bam takes - a per-locus loop over all reads in file order with a dict by name - and the one
generated BAM both allele-counter test files use."""
import functools
import os
import tempfile

import numpy as np

from bamutil import CONSUMES_QUERY, CONSUMES_REF, NT16, effective_cigar, ref_len_of, write_bam

# a numeric chromosome name for the CLI (strcmp puts it in front of chrA); chr1 holds the reads with long CIGARs and is the one
# contig here that the sub-command's per-contig mode (chr1..22, X) runs
REFS = [("chrA", 6000), ("7", 6000), ("chr1", 3000)]
BLOCK_PAYLOAD = 1500                          # records straddle blocks
CHUNK_BYTES = "60000"                         # CTO_ALLELE_CHUNK_BYTES that cuts chrA into several chunks
# name -> (min_bq, min_mq, req_flags, excl_flags)
PARAMS = {"verdict": (20, 20, 0, 2316), "F0": (20, 20, 0, 0), "f2": (20, 20, 2, 2316), "defaults": (20, 35, 3, 3852)}
# two names whose 64-bit FNV-1a hashes (over the name and its NUL) agree in the low 32 bits: 0x....e693b846
COLLIDING_NAMES = ("hc247081", "hc413190")
DEEP_LOCUS = 3005                             # on "7": 2100 reads deep, above the column pile-up's 2048


def _locate(r, p0):
    """(is_del, q) of read r at 0-based reference position p0 inside its span"""
    rp, qp = r["pos"], 0
    for op, n in r["cigar"]:
        if op in CONSUMES_REF:
            if p0 < rp + n:
                return (True, qp) if op in "DN" else (False, qp + (p0 - rp))
            rp += n
        if op in CONSUMES_QUERY:
            qp += n
    raise AssertionError("position outside the read")


def naive_counts(reads, ref_index, positions, min_bq, min_mq, req_flags, excl_flags):
    """int64 [n, 4]: A, C, G, T at the 1-based positions of reference `ref_index`; a read counts with its effective CIGAR (the CG tag's
    operations where the record's field is the long-CIGAR placeholder, bamutil.effective_cigar)"""
    reads = [dict(r, cigar=effective_cigar(r)) for r in reads]
    entered = []
    for r in reads:
        f = r["flag"]
        if r["ref"] != ref_index or r["mapq"] < min_mq or (f & excl_flags) or (f & req_flags) != req_flags:
            continue
        if (req_flags & 2) and bool(f & 32) == bool(f & 16):
            continue
        if (f & 1796) or not r["cigar"]:
            continue
        if ref_len_of(r["cigar"]) == 0 or sum(n for op, n in r["cigar"] if op in CONSUMES_QUERY) != len(r["seq"]):
            continue
        entered.append(r)
    out = np.zeros((len(positions), 4), dtype=np.int64)
    for i, p in enumerate(positions):
        first_c = {}
        for r in entered:
            if not (r["pos"] + 1 <= p <= r["pos"] + ref_len_of(r["cigar"])):
                continue
            is_del, q = _locate(r, p - 1)
            if q < len(r["seq"]):
                c = NT16.index(r["seq"][q])
                bq = r["qual"][q] if r["qual"] is not None else 255
            else:
                c, bq = 0, 0
            counts = (not is_del) and bq >= min_bq
            if r["name"] in first_c:
                counts = counts and c != first_c[r["name"]]
            else:
                first_c[r["name"]] = c
            if counts and c in (1, 2, 4, 8):
                out[i, (1, 2, 4, 8).index(c)] += 1
    return out


def _read(rng, name, flag, ref, pos, cigar, mapq=60, seq=None, qual="random", **kw):
    ql = sum(n for op, n in cigar if op in CONSUMES_QUERY)
    if seq is None:
        seq = "".join(rng.choice(list("ACGT"), size=ql))
    if isinstance(qual, str):
        qual = [int(x) for x in rng.integers(10, 41, size=len(seq))]
    elif isinstance(qual, int):
        qual = [qual] * len(seq)
    return dict(name=name, flag=flag, ref=ref, pos=pos, mapq=mapq, cigar=cigar, seq=seq, qual=qual, **kw)


def _random_cigar(rng, target):
    ops, rl = [], 0
    if rng.random() < 0.2:
        ops.append(("H", int(rng.integers(1, 30))))
    if rng.random() < 0.3:
        ops.append(("S", int(rng.integers(1, 40))))
    while True:
        ops.append((str(rng.choice(list("MMMM=X"))), int(rng.integers(5, 120))))
        rl += ops[-1][1]
        if rl >= target:
            break
        k = rng.random()
        if k < 0.4:
            ops.append(("I", int(rng.integers(1, 6))))
        elif k < 0.8:
            ops.append(("D", int(rng.integers(1, 9))))
            rl += ops[-1][1]
        elif k < 0.9:
            ops.append(("N", int(rng.integers(10, 61))))
            rl += ops[-1][1]
    if rng.random() < 0.3:
        ops.append(("S", int(rng.integers(1, 40))))
    if rng.random() < 0.2:
        ops.append(("H", int(rng.integers(1, 30))))
    return ops


def _many_ops(rng, n_ops, lead=(), turn=0):
    """a CIGAR of n_ops operations after `lead`: short M / = / X runs with an I, D or N between every two of them, in turn
    (`turn` picks the first of them)"""
    ops = list(lead)
    between = "IDN"
    k = turn
    while len(ops) < len(lead) + n_ops:
        if (len(ops) - len(lead)) % 2 == 0:
            ops.append((str(rng.choice(list("MM=X"))), int(rng.integers(2, 9))))
        else:
            ops.append((between[k % 3], int(rng.integers(1, 5))))
            k += 1
    if ops[-1][0] in "IDN":
        ops.append(("M", 3))
    return ops


def make_long_cigar_reads(rng):
    """(reads on chr1, its loci): reads of more than 64 and more than 128 operations, so a pass over 64 operations at a time has
    second and third passes to make; I, D and N sit at and behind operations 64 and 128 (the leading H / S shift them by one and
    two places between reads); loci in every run of 64 operations, none in [400, 1000) so that whole runs go without, and none
    behind 2600 so that reads end well after their last locus"""
    R = 2
    reads = [
        _read(rng, "ops200", 0, R, 20, _many_ops(rng, 200)),
        _read(rng, "ops201h", 16, R, 150, _many_ops(rng, 200, lead=[("H", 5)], turn=1)),
        _read(rng, "ops150cg", 0, R, 300, _many_ops(rng, 150, lead=[("H", 4), ("S", 6)], turn=2), cg_tag=True),
        _read(rng, "ops300", 0, R, 900, _many_ops(rng, 300, turn=1)),
        _read(rng, "ops300cg", 16, R, 1100, _many_ops(rng, 300, lead=[("S", 2)], turn=2), cg_tag=True),
        _read(rng, "ops360late", 0, R, 1700, _many_ops(rng, 360)),          # runs on to ~2900: its last ~90 operations see no locus
    ]
    # same-name reads whose overlap lies behind operation 64 (and 128) of the first: the base of the first at a locus comes from a
    # walk that passes those operations; random bases agree at about one locus in four
    first = _read(rng, "linked", 99, R, 1200, _many_ops(rng, 180), qual=30)
    reads.append(first)
    reads.append(_read(rng, "linked", 147, R, 1200 + 64 * 4 + 30, _many_ops(rng, 140), qual=30))
    reads.append(_read(rng, "linked", 2048 + 99, R, 1200 + 128 * 4 + 20, _many_ops(rng, 70), qual=30))    # a third one, under -F 0
    loci = set(p for p in range(1, 2601) if p % 3 and not 400 <= p < 1000)
    return reads, loci


def _pair(rng, name, pos, cig1, cig2, seq1, seq2, q1=30, q2=30, flags=(99, 147), gap=10):
    return [_read(rng, name, flags[0], 0, pos, cig1, seq=seq1, qual=q1), _read(rng, name, flags[1], 0, pos + gap, cig2, seq=seq2, qual=q2)]


def make_reads_and_loci():
    """(reads in coordinate order, {ref name: sorted 1-based loci})"""
    rng = np.random.default_rng(20260417)
    reads, loci_a = [], set()
    # single-end long reads with every operation, IUPAC / N bases, all over chrA from 50 to ~5900
    for i in range(200):
        pos = int(rng.integers(50, 5200))
        cig = _random_cigar(rng, min(int(rng.integers(300, 1500)), 5750 - pos))
        r = _read(rng, "long%d" % i, 16 * int(rng.integers(0, 2)), 0, pos, cig)
        r["seq"] = "".join(c if rng.random() > 0.05 else str(rng.choice(list("NRYKM="))) for c in r["seq"])
        reads.append(r)
        end = pos + ref_len_of(cig)
        loci_a.update([pos, pos + 1, end, end + 1])              # one base outside, first base, last base, one base outside
    # a read whose D and N hold loci (adjacent ones inside the D)
    reads.append(_read(rng, "dn", 0, 0, 200, [("M", 20), ("D", 5), ("M", 20), ("N", 30), ("M", 20)]))
    loci_a.update([221, 222, 223, 224, 225, 226, 246, 260, 275, 276])
    reads.append(_read(rng, "ends_in_d", 0, 0, 300, [("M", 20), ("D", 3)]))
    loci_a.update([320, 321, 323])
    reads.append(_read(rng, "cg", 0, 0, 400, [("S", 3), ("M", 40), ("I", 2), ("M", 40), ("D", 4), ("=", 30), ("X", 2), ("M", 50)], cg_tag=True))
    reads.append(_read(rng, "noqual", 0, 0, 500, [("M", 120)], qual=None))
    reads.append(_read(rng, "iupac", 0, 0, 600, [("M", 16)], seq="ACGTNRYKMSWBDHV="))
    loci_a.update(range(601, 617))
    for mq in (19, 20, 34, 35):
        reads.append(_read(rng, "mq%d" % mq, 0, 0, 700, [("M", 100)], mapq=mq))
    for bq in (19, 20):
        reads.append(_read(rng, "bq%d" % bq, 0, 0, 800, [("M", 100)], qual=bq))
    loci_a.update([705, 750, 805, 850])
    for fl in (4, 8, 256, 512, 1024, 2048):
        reads.append(_read(rng, "flag%d" % fl, fl, 0, 900, [("M", 100)], qual=35))
    reads.append(_read(rng, "nocigar", 0, 0, 900, [], seq="ACGT", qual=35))
    loci_a.update([905, 950])
    # proper pairs: F/R (kept by -f 2) and F/F (dropped by it)
    reads += _pair(rng, "fr", 1000, [("M", 60)], [("M", 60)], None, None, gap=80)
    reads += _pair(rng, "ff", 1000, [("M", 60)], [("M", 60)], None, None, flags=(67, 131), gap=80)
    loci_a.update([1010, 1050, 1100, 1130])
    # overlapping mates, locus at 0-based P + 20 = base 20 of the first mate, base 10 of the second
    m40 = [("M", 40)]
    d40 = [("M", 20), ("D", 2), ("M", 20)]
    d40b = [("M", 10), ("D", 2), ("M", 30)]
    base = lambda b: "".join(b if k in (10, 20) else "T" for k in range(40))
    reads += _pair(rng, "agree", 1200, m40, m40, base("A"), base("A"))
    reads += _pair(rng, "disagree", 1300, m40, m40, base("A"), base("C"))
    reads += _pair(rng, "lowfirst", 1400, m40, m40, base("G"), base("G"), q1=10)
    reads += _pair(rng, "delfirst", 1500, d40, m40, base("A"), base("A"))
    reads += _pair(rng, "delsecond", 1600, m40, d40b, base("A"), base("C"))
    loci_a.update(p + 21 for p in (1200, 1300, 1400, 1500, 1600))
    # three reads with one name: the third is compared with the first, not the second
    for k, b in enumerate("ACA"):
        reads.append(_read(rng, "trio", 0, 0, 1700 + 5 * k, m40, seq=b * 40, qual=30))
    loci_a.update([1715, 1716])
    # two different names that collide in the low 32 bits of the name hash: both count
    for nm in COLLIDING_NAMES:
        reads.append(_read(rng, nm, 0, 0, 1800, m40, seq="G" * 40, qual=30))
    loci_a.add(1810)
    loci_a.update([10, 20, 5950, 5951, 5990])                   # no coverage before the first and after the last read
    loci_a.update(int(x) for x in rng.integers(1, 6001, size=150))
    # the other contig: a spot deeper than 2048, and a few ordinary reads
    loci_7 = {5, 2999, 3000, DEEP_LOCUS, 3008, 3009, 4000, 5999}
    for i in range(2100):
        reads.append(_read(rng, "deep%d" % i, 16 * (i & 1), 1, 3000, [("M", 8)], qual=int(rng.integers(15, 40))))
    for i in range(20):
        pos = int(rng.integers(0, 5000))
        reads.append(_read(rng, "seven%d" % i, 0, 1, pos, _random_cigar(rng, 600)))
        loci_7.update([pos + 1, pos + 300])
    many, loci_1 = make_long_cigar_reads(rng)
    reads += many
    reads.sort(key=lambda r: (r["ref"], r["pos"]))                # stable: pairs and trios keep their order
    keep = lambda s: sorted(p for p in s if 1 <= p <= 6000)
    return reads, {"chrA": keep(loci_a), "7": keep(loci_7), "chr1": keep(loci_1)}


def check_case(reads, loci):
    """the generated case holds what the tests rely on (run once, when the case is built)"""
    many = [r for r in reads if r["ref"] == 2]
    assert max(len(r["cigar"]) for r in many) > 256 and sum(len(r["cigar"]) > 128 for r in many) >= 5
    assert any(r.get("cg_tag") and len(r["cigar"]) > 128 for r in many)
    for lo in (64, 128):                                          # I, D and N at the first operation of a later pass and behind it
        at = {r["cigar"][lo][0] for r in many if len(r["cigar"]) > lo} | {r["cigar"][lo - 1][0] for r in many if len(r["cigar"]) > lo}
        assert set("IDN") <= at, at
    pos = np.array(loci["chr1"])
    for r in many:                                                # loci inside every run of 64 operations that lies in front of 2600
        rp = r["pos"]
        for k0 in range(0, len(r["cigar"]), 64):
            span = ref_len_of(r["cigar"][k0:k0 + 64])
            if rp + span <= 2600 and not (400 <= rp + 1 and rp + span < 1000):
                assert ((pos > rp) & (pos <= rp + span)).any() or 400 <= rp + 1 < 1000 or 400 <= rp + span < 1000, (r["name"], k0)
            rp += span
    linked = [r for r in many if r["name"] == "linked"]
    ops_before = lambda r, p0: next(k for k in range(len(r["cigar"]) + 1) if r["pos"] + ref_len_of(r["cigar"][:k + 1]) > p0)
    assert ops_before(linked[0], linked[1]["pos"]) >= 64 and ops_before(linked[0], linked[2]["pos"]) >= 128
    assert linked[0]["pos"] + ref_len_of(linked[0]["cigar"]) > linked[2]["pos"] + 50


_CASE = {}


def case():
    """the generated BAM (written once per process into a temporary directory), its reads and loci"""
    if not _CASE:
        reads, loci = make_reads_and_loci()
        d = tempfile.mkdtemp(prefix="allele_counter_")
        bam = os.path.join(d, "t.bam")
        check_case(reads, loci)
        write_bam(bam, REFS, reads, block_payload=BLOCK_PAYLOAD)
        _CASE.update(bam=bam, dir=d, reads=reads, loci=loci)
    return _CASE


@functools.lru_cache(maxsize=None)
def expected(ctg, params):
    """naive counts of one contig's loci under PARAMS[params]: computed once, shared by every test (read-only)"""
    c = case()
    out = naive_counts(c["reads"], [n for n, _ in REFS].index(ctg), c["loci"][ctg], *PARAMS[params])
    out.setflags(write=False)
    return out


def loci_file_lines():
    """a loci file over both contigs, out of order, with a repeated locus, extra columns and the numeric name written three ways"""
    c = case()
    lines = ["chrA\t%d" % p for p in c["loci"]["chrA"][::-1]]
    lines += ["%s\t%d\tA\tG" % (("7", "07", "007")[i % 3], p) for i, p in enumerate(c["loci"]["7"])]
    lines.insert(3, "chrA %d" % c["loci"]["chrA"][40])           # a repeat, space separated
    lines.append("7\t%d" % DEEP_LOCUS)                             # a repeat of the deep locus
    return lines


def expected_table(params):
    """the bytes alleleCounter's table has for loci_file_lines(): sorted by strcmp(chr), pos; a repeat prints zeros"""
    c = case()
    rows = []
    for ctg in ("7", "chrA"):                                     # no chr1 line in loci_file_lines()
        pos = list(c["loci"][ctg]) + ([DEEP_LOCUS] if ctg == "7" else [c["loci"]["chrA"][40]])
        want = {p: expected(ctg, params)[i] for i, p in enumerate(c["loci"][ctg])}
        seen = set()
        for p in sorted(pos):
            r = want[p] if p not in seen else np.zeros(4, dtype=np.int64)
            seen.add(p)
            rows.append("%s\t%d\t%d\t%d\t%d\t%d\t%d\n" % (ctg, p, r[0], r[1], r[2], r[3], r.sum()))
    return "#CHR\tPOS\tCount_A\tCount_C\tCount_G\tCount_T\tGood_depth\n" + "".join(rows)
