"""Test-only: a deliberately naive restatement of the AF-tally rules (the list at the top of csrc/aftally.hip) over the read dicts
tests/bamutil.py:write_bam takes - per locus a loop over all reads in file order that builds the column `samtools mpileup` would print -
and the one generated case both cal_af_distribution test files and tests/golden/gen_cal_af.py use.  mpileup_row() is the text of that
column (the seven columns of `samtools mpileup --output-extra HP -r ctg:p-p`, with `^`, `$`, `>` and `<`); tally_of_row() is what
src/cal_af_distribution.py:44-115 makes of such a row, restated; naive_tally() is the two together."""
import functools
import hashlib
import json
import os
import struct
import tempfile

import numpy as np

from allelecountutil import _many_ops, _read
from bamutil import CONSUMES_QUERY, CONSUMES_REF, effective_cigar, ref_len_of, write_bam

SEED = 20261019
REFS = [("chrA", 6000), ("chrB", 5200), ("chrC", 3000)]
BLOCK_PAYLOAD = 1500                          # records straddle blocks
CHUNK_BYTES = "40000"                         # CTO_AF_CHUNK_BYTES that cuts chrA into several chunks
MIN_MQ, EXCL_FLAGS = 20, 2316
LOW_MAX_DEPTH = 16                            # the GPU tests' cap: one planted locus is deeper, every other locus stays below
MAX_INS = 64                                  # CTO_AF_MAX_INS
OTHER_SKIP_LOCI = 4                           # loci under a reference skip on chrA and on chrC (chrB: the three planted ones)
INT_TYPES = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}


# ------------------------------------------------------------------------------------------ the naive pile-up
def hp_text(aux):
    """what --output-extra HP prints for a record with these auxiliary bytes: the first HP field of an integer type in decimal, `*` without
    one.  The walk is the SAM specification's (4.2.4); it ends at an unknown type or a field that does not fit."""
    i, n = 0, len(aux)
    while i + 3 <= n:
        tag, ty = aux[i:i + 2], chr(aux[i + 2])
        i += 3
        if ty in "AcC":
            size = 1
        elif ty in "sS":
            size = 2
        elif ty in "iIf":
            size = 4
        elif ty in "ZH":
            nul = aux.find(b"\0", i)
            if nul < 0:
                break
            size = nul + 1 - i
        elif ty == "B":
            if i + 5 > n:
                break
            size = 5 + struct.unpack_from("<I", aux, i + 1)[0] * {"c": 1, "C": 1, "s": 2, "S": 2}.get(chr(aux[i]), 4)
        else:
            break
        if i + size > n:
            break
        if tag == b"HP" and ty in INT_TYPES:
            return str(struct.unpack_from(INT_TYPES[ty], aux, i)[0])
        i += size
    return "*"


def entered(reads, ref_index, min_mq=MIN_MQ, excl_flags=EXCL_FLAGS):
    """the reads of one contig that enter the pile-up, in file order, with their effective CIGAR, reference end and HP text"""
    from bamutil import _aux_bytes
    out = []
    for r in reads:
        f = r["flag"]
        if r["ref"] != ref_index or (f & excl_flags) or (f & 4) or r["mapq"] < min_mq or ((f & 1) and not (f & 2)):
            continue
        cigar = effective_cigar(r)
        if not cigar or not r["seq"] or sum(n for op, n in cigar if op in CONSUMES_QUERY) != len(r["seq"]) or ref_len_of(cigar) == 0:
            continue
        out.append(dict(r, cigar=cigar, end=r["pos"] + ref_len_of(cigar), hp=hp_text(_aux_bytes(r))))
    return out


def token_at(r, p0):
    """the read's text in the column of 0-based position p0 (inside its span), without `^` and `$`"""
    rev = bool(r["flag"] & 16)
    rp, qp, ops = r["pos"], 0, r["cigar"]
    for i, (op, n) in enumerate(ops):
        if op in CONSUMES_REF and p0 < rp + n:
            if op == "N":
                return "<" if rev else ">"
            if op == "D":
                return "*"
            b = r["seq"][qp + p0 - rp]
            tok = b if b in "ACGT" else "N"
            if p0 == rp + n - 1:
                j = i + 1
                while j < len(ops) and ops[j][0] == "P":
                    j += 1
                if j < len(ops) and ops[j][0] == "I":
                    q1 = qp + n
                    tok += "+%d%s" % (ops[j][1], "".join("N" if c == "=" else c for c in r["seq"][q1:q1 + ops[j][1]]))
                elif j < len(ops) and ops[j][0] == "D":
                    tok += "-%d%s" % (ops[j][1], "N" * ops[j][1])
            return tok.lower() if rev else tok
        if op in CONSUMES_REF:
            rp += n
        if op in CONSUMES_QUERY:
            qp += n
    raise AssertionError("position outside the read")


def column(ent, pos, max_depth=8000):
    """the first max_depth entered reads that cover 1-based `pos`, in file order"""
    cov = [r for r in ent if r["pos"] < pos <= r["end"]]
    return cov[:max_depth] if max_depth > 0 else cov


def mpileup_row(ent, ctg, pos, with_hp, max_depth=8000):
    """the row `samtools mpileup [--output-extra HP] -r ctg:pos-pos` prints ("" when no read covers the position)"""
    cov = column(ent, pos, max_depth)
    if not cov:
        return ""
    bases = ""
    for r in cov:
        if r["pos"] + 1 == pos:
            bases += "^" + chr(min(r["mapq"], 93) + 33)
        bases += token_at(r, pos - 1)
        if r["end"] == pos:
            bases += "$"
    cols = [ctg, str(pos), "N", str(len(cov)), bases, "I" * len(cov)]
    if with_hp:
        cols.append(",".join(r["hp"] for r in cov))
    return "\t".join(cols) + "\n"


def match_alt_of(ref_base, alt_base):
    """src/cal_af_distribution.py:93-97"""
    alt_base = alt_base.upper()
    if len(ref_base) == 1 and len(alt_base) > 1:
        return alt_base[0] + "+" + alt_base[1:]
    if len(ref_base) > 1 and len(alt_base) == 1:
        return ref_base[0].upper() + "-" + "N" * (len(ref_base) - 1)
    return alt_base


def tally_of_row(row, match_alt):
    """[depth, alt, h0, h1, h2, a0, a1, a2] as src/cal_af_distribution.py:44-115 reads them off a row; IndexError where it raises"""
    cols = row.rstrip().split("\t")
    if len(cols) < 5:
        return [0] * 8
    text, i, entries = cols[4], 0, []
    while i < len(text):
        c = text[i]
        if c in "+-":
            j = i + 1
            while text[j].isdigit():
                j += 1
            n = int(text[i + 1:j])
            entries[-1] += c + text[j:j + n]
            i = j + n
            continue
        if c == "^":
            i += 2
            continue
        if c in "ACGTNacgtn#*":
            entries.append(c)
        i += 1
    entries = [e.upper() for e in entries]
    out = [len(entries), sum(e == match_alt for e in entries), 0, 0, 0, 0, 0, 0]
    if len(cols) >= 7:
        for e, hap in zip(entries, cols[6].split(",")):
            h = int(hap) if hap in "12" else 0
            out[5 + h] += 1                                       # IndexError for "12", as the reference's list has three places
            out[2 + h] += e == match_alt
    return out


def naive_tally(ent, ctg, pos, ref_base, alt_base, with_hp, max_depth=8000):
    return tally_of_row(mpileup_row(ent, ctg, pos, with_hp, max_depth), match_alt_of(ref_base, alt_base))


def order_dependent(ent, pos, ref_base, alt_base, with_hp, max_depth):
    """whether the device path has to hand the locus to the host path (the three kinds csrc/aftally.hip lists; no HP 12 in this case)"""
    cov = [r for r in ent if r["pos"] < pos <= r["end"]]
    if max_depth > 0 and len(cov) > max_depth:
        return True
    if len(ref_base) == 1 and len(alt_base) - 1 > MAX_INS:
        return True
    return bool(with_hp) and any(token_at(r, pos - 1) in "<>" for r in cov)


# ------------------------------------------------------------------------------------------ the case
def hp_aux(ty, val, lead=""):
    """auxiliary bytes: the fields `lead` names (Z H A f B: one of each kind a walker has to step over), then HP of integer type `ty`"""
    fields = {"Z": b"XAZ" + b"HPC\x01HPi" + b"\0", "H": b"XHH" + b"1AE301" + b"\0", "A": b"xsA" + b"+", "f": b"xff" + struct.pack("<f", 1.5),
              "B": b"mlBC" + struct.pack("<I", 3) + bytes([1, 2, 3]) + b"xbBs" + struct.pack("<Ihh", 2, -5, 7) + b"xiBI" + struct.pack("<II", 1, 12)}
    aux = b"".join(fields[k] for k in lead)
    if ty is not None:
        aux += b"HP" + ty.encode() + struct.pack(INT_TYPES[ty], val)
    return aux + b"NMi" + struct.pack("<i", 2)


def _short_cigar(rng):
    """two to four aligned runs of 4 .. 14 bases with an I, D, N or P + I between them, clips at the ends now and then: about 30 bases"""
    ops = [("S", int(rng.integers(1, 6)))] if rng.random() < 0.2 else []
    for k in range(int(rng.integers(2, 5))):
        if k:
            x = rng.random()
            if x < 0.4:
                ops.append(("I", int(rng.integers(1, 5))))
            elif x < 0.8:
                ops.append(("D", int(rng.integers(1, 5))))
            elif x < 0.9:
                ops.append(("N", int(rng.integers(3, 12))))
            else:
                ops += [("P", 1), ("I", int(rng.integers(1, 4)))]
        ops.append((str(rng.choice(list("MMM=X"))), int(rng.integers(4, 15))))
    if rng.random() < 0.2:
        ops.append(("H", int(rng.integers(1, 9))))
    return ops


def _alternating(n_ops, lead=(), seps="ID", at=None):
    """`lead`, then M3 and a separator in turn, n_ops operations in all, ending in an M; at = {operation index: (op, n)} overrides"""
    ops = list(lead)
    k = 0
    while len(ops) < n_ops:
        if (len(ops) - len(lead)) % 2 == 0:
            ops.append(("M", 3))
        else:
            ops.append((seps[k % len(seps)], 2))
            k += 1
    if ops[-1][0] != "M":
        ops.append(("M", 3))
    for i, o in (at or {}).items():
        ops[i] = o
    return ops


def _ref_pos_of_op(r, k):
    """0-based reference position of the last base of operation k of read r"""
    return r["pos"] + ref_len_of(r["cigar"][:k + 1]) - 1


def make_case():
    """-> dict(reads, variants): reads in coordinate order; variants = [(ctg, pos, REF, ALT)] in truth-file order (not sorted), about
    300 of them, each planted situation with a name in `planted`"""
    rng = np.random.default_rng(SEED)
    reads, planted = [], {}                                      # planted: name -> (ctg, pos, REF, ALT)
    hp_kinds = [(None, 0, ""), ("C", 1, ""), ("C", 2, "Z"), ("c", 1, "ZH"), ("s", 2, "A"), ("S", 1, "f"), ("i", 2, "B"), ("I", 1, "ZHAfB"),
                ("C", 0, ""), ("i", 3, "B"), ("c", -1, ""), ("S", 2, "BZ")]
    some_hp = lambda: hp_aux(*hp_kinds[int(rng.integers(0, len(hp_kinds)))])
    # ---- chrA: ~2300 short reads, every operation, IUPAC bases, both strands, random HP of every type: cover stays near 10
    for i in range(2300):
        pos = int(rng.integers(20, 5850))
        cig = _short_cigar(rng)
        r = _read(rng, "a%d" % i, 16 * int(rng.integers(0, 2)), 0, pos, cig, aux=some_hp())
        r["seq"] = "".join(c if rng.random() > 0.03 else str(rng.choice(list("NRYKM="))) for c in r["seq"])
        reads.append(r)
    # ---- chrB: the planted situations, one per window of 100 bases, three plain reads under each so that columns are mixed
    B = 1

    def window(w, rs):
        for r in rs:
            reads.append(r)
        for k in range(3):
            reads.append(_read(rng, "bg%d_%d" % (w, k), 16 * (k & 1), B, w + 5 * k, [("M", 90)], aux=some_hp()))

    acgt = lambda n: "".join(rng.choice(list("ACGT"), size=n))
    m20 = "ACGTACGTACGTACGTACGA"                                  # 20 bases ending in A: the anchor
    tail = "TTGCATTGCATTGCATTGCA"
    # first and last base of a read
    window(100, [_read(rng, "ends", 0, B, 110, [("M", 50)], aux=hp_aux("C", 1))])
    planted["first_base"] = ("chrB", 111, "A", "C")
    planted["last_base"] = ("chrB", 160, "A", "G")
    # insertions at one anchor (0-based 219): equal to the ALT, one base longer, same length other bases, reverse strand, behind P, none
    ins = lambda name, flag, seq_ins, hp, cig=None: _read(rng, name, flag, B, 200, cig or [("M", 20), ("I", len(seq_ins)), ("M", 20)],
                                                        seq=m20 + seq_ins + tail, aux=hp)
    window(200, [ins("ins_eq", 0, "GAT", hp_aux("C", 1, "Z")), ins("ins_long", 0, "GATC", hp_aux("s", 2, "H")), ins("ins_diff", 0, "GAA", hp_aux("i", 1)),
                 ins("ins_rev", 16, "GAT", hp_aux("S", 2, "f")), ins("ins_p", 0, "GAT", hp_aux("I", 2, "B"), [("M", 20), ("P", 2), ("I", 3), ("M", 20)]),
                 ins("ins_iupac", 0, "GRT", hp_aux("c", 2, "A")), _read(rng, "ins_none", 0, B, 200, [("M", 40)], seq=m20 + tail, aux=hp_aux(None, 0))])
    planted["ins"] = ("chrB", 220, "A", "AGAT")
    # I directly behind S: not reported
    window(300, [_read(rng, "s_then_i", 0, B, 310, [("S", 5), ("I", 3), ("M", 40)], aux=hp_aux("C", 2))])
    planted["behind_s_i"] = ("chrB", 311, "A", "ACCC")
    # deletions behind one anchor (0-based 419): del_len 3, 2 and 4; an anchor base that is not REF[0]; the locus inside the D
    dele = lambda name, n, seq0=m20, flag=0: _read(rng, name, flag, B, 400, [("M", 20), ("D", n), ("M", 20)], seq=seq0 + tail, aux=some_hp())
    window(400, [dele("del3", 3), dele("del2", 2), dele("del4", 4), dele("del3_rev", 3, flag=16), dele("del3_other_anchor", 3, seq0=m20[:-1] + "C")])
    planted["del"] = ("chrB", 420, "ACCC", "A")
    planted["inside_del"] = ("chrB", 421, "C", "T")
    planted["del_as_snv"] = ("chrB", 520, "A", "C")              # filled below: a plain base where others have a suffix
    window(500, [_read(rng, "snv_plain", 0, B, 500, [("M", 40)], seq=m20[:-1] + "C" + tail, aux=hp_aux("C", 1)),
                 _read(rng, "snv_with_del", 0, B, 500, [("M", 20), ("D", 1), ("M", 20)], seq=m20[:-1] + "C" + tail, aux=hp_aux("C", 1))])
    # HP of every integer type behind fields of every other type; absent; 0 and 3
    window(600, [_read(rng, "hp_%s" % (ty or "none"), 0, B, 600, [("M", 60)], seq="C" * 60, aux=hp_aux(ty, v, lead)) for ty, v, lead in hp_kinds])
    planted["hp_types"] = ("chrB", 630, "A", "C")
    # overlapping proper pair, an orphan, MAPQ 19 and 20, every flag of 2316, a duplicate and a QC failure (both count)
    window(700, [_read(rng, "pair", 99, B, 700, [("M", 50)], seq="G" * 50, aux=hp_aux("C", 1)), _read(rng, "pair", 147, B, 720, [("M", 50)], seq="G" * 50, aux=hp_aux("C", 1)),
                 _read(rng, "orphan", 65, B, 710, [("M", 50)], seq="G" * 50), _read(rng, "mq19", 0, B, 712, [("M", 50)], seq="G" * 50, mapq=19),
                 _read(rng, "mq20", 0, B, 714, [("M", 50)], seq="G" * 50, mapq=20)] +
           [_read(rng, "flag%d" % f, f, B, 716, [("M", 50)], seq="G" * 50, aux=hp_aux("C", 2)) for f in (4, 8, 256, 2048, 1024, 512)])
    planted["filters"] = ("chrB", 745, "A", "G")
    # a CG-tag CIGAR
    window(800, [_read(rng, "cg", 0, B, 800, [("S", 3), ("M", 20), ("I", 2), ("M", 20), ("D", 4), ("=", 10), ("X", 2), ("M", 20)], cg_tag=True)])
    planted["cg_ins"] = ("chrB", 820, "A", reads[-4]["seq"][22:25])       # the anchor (S3 + M20) and the two inserted bases
    # reference skips: the skipping read lies between reads of different HP, so the shift moves counts between haplotypes
    for w in (900, 1000, 1100):
        window(w, [_read(rng, "hp1_%d" % w, 0, B, w, [("M", 80)], seq="T" * 80, aux=hp_aux("C", 1)),
                   _read(rng, "skip_%d" % w, 16 * (w == 1000), B, w + 2, [("M", 10), ("N", 30), ("M", 20)], aux=hp_aux("C", 2)),
                   _read(rng, "hp2_%d" % w, 0, B, w + 4, [("M", 70)], seq="T" * 70, aux=hp_aux("s", 2)),
                   _read(rng, "hp0_%d" % w, 0, B, w + 6, [("M", 70)], seq="A" * 70)])
        planted["skip_%d" % w] = ("chrB", w + 25, "A", "T")
    planted["before_skip"] = ("chrB", 912, "A", "T")             # the last M base before the N: no suffix, an entry
    # a locus deeper than LOW_MAX_DEPTH: 40 reads, the ALT among the later ones only
    window(1300, [_read(rng, "deep%d" % i, 16 * (i & 1), B, 1300 + (i % 7), [("M", 40)], seq=("A" if i < 20 else "G") * 40, aux=hp_aux("C", 1 + (i & 1)))
                  for i in range(40)])
    planted["deep"] = ("chrB", 1320, "A", "G")
    # an insertion ALT longer than the kernel compares, and a read that has it
    long_ins = acgt(MAX_INS + 6)
    window(1500, [_read(rng, "long_ins", 0, B, 1500, [("M", 20), ("I", len(long_ins)), ("M", 20)], seq=m20 + long_ins + tail, aux=hp_aux("C", 2)),
                  _read(rng, "ins64", 0, B, 1600, [("M", 20), ("I", MAX_INS), ("M", 20)], seq=m20 + long_ins[:MAX_INS] + tail, aux=hp_aux("C", 1))])
    planted["long_ins"] = ("chrB", 1520, "A", "A" + long_ins)
    planted["ins64"] = ("chrB", 1620, "A", "A" + long_ins[:MAX_INS])        # the longest the kernel compares: stays on the device
    for k in range(3):
        reads.append(_read(rng, "bg1600_%d" % k, 0, B, 1600 + 5 * k, [("M", 90)], aux=some_hp()))
    # more than 64 and more than 128 operations; the last M base before an I is operation 63 (the I is lane 0 of the next pass), operation 64,
    # and operation 127 with a P between it and the I
    long_a = _read(rng, "ops150", 0, B, 2000, _alternating(150, lead=[("S", 2)], at={64: ("I", 2), 128: ("P", 1), 129: ("I", 3)}), aux=hp_aux("I", 1, "ZB"))
    long_b = _read(rng, "ops100", 16, B, 2600, _alternating(100, at={65: ("I", 4)}), aux=hp_aux("c", 2))
    long_c = _read(rng, "ops300cg", 0, B, 3000, _alternating(300, lead=[("H", 4)], seps="IDN"), cg_tag=True)
    for r in (long_a, long_b, long_c):
        window(r["pos"], [r])
    ins_after = lambda r, k, j: ("chrB", _ref_pos_of_op(r, k) + 1, "A",
                                 r["seq"][sum(n for op, n in r["cigar"][:k + 1] if op in CONSUMES_QUERY) - 1:
                                          sum(n for op, n in r["cigar"][:j + 1] if op in CONSUMES_QUERY)])
    planted["ins_across_64"] = ins_after(long_a, 63, 64)
    planted["ins_p_across_128"] = ins_after(long_a, 127, 129)
    planted["ins_at_64"] = ins_after(long_b, 64, 65)
    # ---- chrC: reads of many operations over one another, loci drawn from what they show
    for i in range(40):
        reads.append(_read(rng, "c%d" % i, 16 * (i & 1), 2, 30 + 50 * i, _many_ops(rng, int(rng.integers(40, 200)), turn=i), aux=some_hp(), cg_tag=(i % 9 == 4)))
    reads.sort(key=lambda r: (r["ref"], r["pos"]))                # stable
    # ---- variants: the planted ones, then loci drawn per contig among positions whose cover stays below the lowered cap; the allele is
    # one the column shows (a base, an insertion, a deletion) three times in four, a random one otherwise
    variants = list(planted.values())
    taken = set((c, p) for c, p, _, _ in variants)
    for ci, (ctg, n_draw) in enumerate((("chrA", 170), ("chrB", 50), ("chrC", 60))):
        ent = entered(reads, ci)
        cand = [int(p) for p in rng.permutation(np.arange(1, REFS[ci][1] + 1)) if (ctg, int(p)) not in taken]
        drawn = skips = 0
        for p in cand:
            if drawn == n_draw:
                break
            cov = column(ent, p)
            under_skip = any(token_at(r, p - 1) in "<>" for r in cov)
            if len(cov) > LOW_MAX_DEPTH or (under_skip and (ctg == "chrB" or skips == OTHER_SKIP_LOCI)):
                continue                                          # the planted deep locus and skip loci stay the only ones of their kind on chrB;
            skips += under_skip                                   # OTHER_SKIP_LOCI on each of the other contigs
            if not cov and rng.random() < 0.9:
                continue                                          # and a few loci without cover
            toks = [token_at(r, p - 1).upper() for r in cov if token_at(r, p - 1) not in "<>*"]
            indel = [t for t in toks if len(t) > 1]
            if indel and rng.random() < 0.75:
                t = indel[int(rng.integers(0, len(indel)))]
                digits = "".join(ch for ch in t[2:] if ch.isdigit())
                body = t[2 + len(digits):]
                ref_alt = (t[0], t[0] + body) if t[1] == "+" else (t[0] + "C" * int(digits), t[0])
            elif toks and rng.random() < 0.75:
                ref_alt = ("N", toks[int(rng.integers(0, len(toks)))][0])
            else:
                ref_alt = ("A", "ACGT"[int(rng.integers(0, 4))])
            variants.append((ctg, p) + ref_alt)
            drawn += 1
    order = rng.permutation(len(variants))
    variants = [variants[int(i)] for i in order]
    return dict(reads=reads, variants=variants, planted=planted)


def check_case(c):
    """the generated case holds what the tests rely on (run once, when the case is built)"""
    ent = {ctg: entered(c["reads"], i) for i, (ctg, _) in enumerate(REFS)}
    P = c["planted"]
    t = lambda name, with_hp=True, md=8000: naive_tally(ent[P[name][0]], *P[name], with_hp, md)
    assert t("ins")[:2] == [10, 3], t("ins")                     # ins_eq, ins_rev, ins_p of seven reads + three plain
    assert t("del")[1] == 2 and t("inside_del")[0] == t("del")[0]
    assert 1 <= t("del_as_snv")[1] <= 4                          # the read whose C carries a deletion is not the SNV (3 random reads may be)
    assert t("behind_s_i")[1] == 0 and t("ins_across_64")[1] == 1 and t("ins_p_across_128")[1] == 1 and t("ins_at_64")[1] == 1
    assert t("long_ins")[1] == 1 and t("ins64")[1] == 1 and t("cg_ins")[1] == 1
    assert t("first_base")[0] == 4 and t("last_base")[0] >= 2
    got = t("filters")                                            # pair x 2, mq20, dup, qcfail + 3 plain; the orphan, mq19 and 2316's flags do not enter
    assert got[0] == 8, got
    hp = t("hp_types")
    assert hp[0] == 15 and min(hp[5:8]) >= 4, hp                 # four reads of each haplotype, and three random ones
    for w in (900, 1000, 1100):                                   # the shift changes the tallies: with the HP values re-paired they differ
        row = mpileup_row(ent["chrB"], "chrB", w + 25, True)
        cols = row.rstrip().split("\t")
        keep = [h for tok, h in zip(_tokens(ent["chrB"], w + 25), cols[6].split(",")) if tok not in "<>"]
        fixed = "\t".join(cols[:4] + [cols[4].replace(">", "").replace("<", ""), cols[5][:len(keep)], ",".join(keep)])
        assert tally_of_row(fixed, "T") != tally_of_row(row, "T")
    assert t("deep")[0] > LOW_MAX_DEPTH and t("deep", md=LOW_MAX_DEPTH) != t("deep")
    n_ops = sorted(len(r["cigar"]) for r in c["reads"])
    assert n_ops[-1] > 128 and sum(n > 64 for n in n_ops) >= 10
    for ctg, p, ref, alt in c["variants"]:
        if (ctg, p) != P["deep"][:2]:
            assert len(column(ent[ctg], p)) <= LOW_MAX_DEPTH, (ctg, p)
    assert len(set((ctg, p) for ctg, p, _, _ in c["variants"])) == len(c["variants"]) and 280 <= len(c["variants"]) <= 330
    assert len(c["reads"]) > 2000


def _tokens(ent, pos):
    return [token_at(r, pos - 1) for r in column(ent, pos)]


_CASE = {}


def case():
    """the generated BAM (written once per process into a temporary directory), its reads, variants and entered reads per contig"""
    if not _CASE:
        c = make_case()
        check_case(c)
        d = tempfile.mkdtemp(prefix="cal_af_")
        bam = os.path.join(d, "t.bam")
        write_bam(bam, REFS, c["reads"], block_payload=BLOCK_PAYLOAD)
        _CASE.update(c, bam=bam, dir=d, entered={ctg: entered(c["reads"], i) for i, (ctg, _) in enumerate(REFS)})
    return _CASE


def reads_digest(reads):
    """SHA-256 over every field of every read, in order: what tests/golden/cal_af.json.gz records of the case it was made from"""
    return hashlib.sha256(json.dumps([[r[k] if not isinstance(r[k], bytes) else r[k].hex() for k in sorted(r)] for r in reads]).encode()).hexdigest()


def contig_loci(ctg):
    """(sorted 1-based loci, [(REF, ALT)]) of one contig's variants"""
    vs = sorted((p, ref, alt) for c, p, ref, alt in case()["variants"] if c == ctg)
    return [p for p, _, _ in vs], [(ref, alt) for _, ref, alt in vs]


@functools.lru_cache(maxsize=None)
def expected(ctg, with_hp, max_depth):
    """naive tallies of one contig's loci, int32 [n, 8]: computed once, shared by every test (read-only)"""
    ent = case()["entered"][ctg]
    loci, ra = contig_loci(ctg)
    out = np.array([naive_tally(ent, ctg, p, ref, alt, with_hp, max_depth) for p, (ref, alt) in zip(loci, ra)], dtype=np.int32)
    out.setflags(write=False)
    return out


def expected_host_loci(ctg, with_hp, max_depth):
    ent = case()["entered"][ctg]
    loci, ra = contig_loci(ctg)
    return sum(order_dependent(ent, p, ref, alt, with_hp, max_depth) for p, (ref, alt) in zip(loci, ra))


# ------------------------------------------------------------------------------------------ the fixture
@functools.lru_cache(maxsize=None)
def golden():
    """tests/golden/cal_af.json.gz (gen_cal_af.py: the reference's run on this case)"""
    import gzip
    return json.load(gzip.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cal_af.json.gz"), "rt"))


def write_vcfs(d):
    """the fixture's two VCFs (the truth file also gzip-compressed) into directory d, under the names its configurations use"""
    import gzip
    g = golden()
    open(os.path.join(d, "truth.vcf"), "w").write(g["truth_vcf"])
    with gzip.open(os.path.join(d, "truth.vcf.gz"), "wt") as f:
        f.write(g["truth_vcf"])
    open(os.path.join(d, "input.vcf"), "w").write(g["input_vcf"])


def config_argv(cf, d, output_path, where):
    """the command line of one fixture configuration, on the case's BAM and the files write_vcfs(d) wrote"""
    ns = cf["namespace"]
    argv = ["--tumor_bam_fn", case()["bam"], "--truth_vcf_fn", os.path.join(d, ns["truth_vcf_fn"]), "--input_vcf_fn", os.path.join(d, ns["input_vcf_fn"]),
            "--phase_output", str(ns["phase_output"]), "--threads", "2", "--samtools", "samtools", "--where", where]
    for k in ("ctg_name", "truth_filter_tag", "input_filter_tag"):
        if ns[k] is not None:
            argv += ["--" + k, ns[k]]
    return argv + (["--output_path", str(output_path)] if output_path else [])


# ------------------------------------------------------------------------------------------ the two VCFs
def vcf_texts():
    """(truth VCF, input VCF) of the case.  The truth file holds every variant as a PASS row in `variants` order, and around them the rows
    VcfReader treats specially: a NonPass row (dropped under --truth_filter_tag PASS), a 0/0 row, a repeated key (the last row stands),
    `*` ALTs (one well-formed, one not), a genotype that does not parse (kept), a two-ALT row (the first is used), a lower-case ALT.  The
    input file holds every fifth truth variant with DP and AF - one with AF * DP = 2.5, which Python rounds to 2 - a few of them 0/0 (so
    that their truth variants are piled up after all), and a call of its own; its header ends in TUMOR and its rows have a column more."""
    c = case()
    head = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n"
    row = lambda ctg, p, ref, alt, flt="PASS", gt="0/1", rest="": "%s\t%d\t.\t%s\t%s\t10\t%s\t.\tGT%s\t%s%s\n" % (ctg, p, ref, alt, flt, ":X" if rest else "", gt, rest)
    truth = head
    vs = c["variants"]
    free = [p for p in range(4000, 4400, 20)]                    # chrB positions no read reaches: rows of zeros
    truth += row("chrB", free[0], "A", "C", flt="NonPass")
    truth += row("chrB", free[1], "A", "C", gt="0/0")
    truth += row("chrB", free[2], "A", "G")                      # replaced by the row at the end
    for i, (ctg, p, ref, alt) in enumerate(vs):
        if i % 40 == 7 and len(alt) == 1:
            alt = alt.lower()
        if i % 40 == 11:
            alt = alt + ",T"
        truth += row(ctg, p, ref, alt, gt=("1|0", "0/1", "1/1", "./1")[i % 4])
    truth += row("chrB", free[3], "A", "C,*", gt="1/2")          # -> ALT C
    truth += row("chrB", free[4], "A", "C,*", gt="0/1")          # error with variant representation: dropped
    truth += row("chrB", free[5], "A", "T", gt="1")              # does not parse: kept
    truth += row("chrB", free[2], "AT", "A", rest=":7")          # the repeat
    truth += row("chrC", 2990, "A", "C")                         # no cover
    inp = head.replace("SAMPLE", "TUMOR")
    fmt = lambda ctg, p, dp, af, gt="0/1": "%s\t%d\t.\tA\tC\t12\tPASS\t.\tGT:GQ:DP:AF\t%s:12:%d:%s\t0/0\n" % (ctg, p, gt, dp, af)
    for i, (ctg, p, ref, alt) in enumerate(vs):
        if i % 5 == 3:                                            # the header ends in TUMOR: the genotype is the last column but one
            inp += fmt(ctg, p, 10 if i == 3 else 10 + i % 30, "0.25" if i == 3 else "%.4f" % ((i % 17) / 17.0), gt="0/0" if i % 25 == 8 else "0/1")
    inp += fmt("chrA", 5999, 30, "0.5")
    return truth, inp
