"""Synthetic inputs of the Verdict sub-chain allele counts -> BAF -> germline genotypes (src/verdict/get_logr_and_baf.py and
src/verdict/predict_germline_genotypes.py of the reference): input synthesis for gen_verdict_gg.py and for the tests, which regenerate the
inputs from the specs and check them against the stored SHA-256.  The product never imports this.

count_files(spec): per contig a 1000G-style allele file (position, a0, a1 with 1..4 = A, C, G, T), an alleleCounter table of the tumour
and one of the normal, and the contig list.  The tables hold every ref / alt letter pair, loci that the allele file does not have, tumour
rows whose ref + alt total is 0 (the other two letters are not), normal totals of 8, 9, 10 and 11, a position that occurs twice in a
count table and one that occurs twice in the allele file.

baf_files(spec): a BAF table (and a logR table with the same keys) laid out so that the number of UNDECIDED probes of every run of
chromosome names is the spec's.  Homozygous probes have a mirrored BAF of at most 2 / depth, heterozygous ones are binomial around 0.5,
both printed as alt / depth with depths of 200 - 400; the row count n is chosen with round(0.65 n) = n - (undecided), so that with the
reference's default proportionHomo the quantile is the smallest heterozygous value: exactly the heterozygous probes are undecided."""
import hashlib
import random

ACGT = "ACGT"
COUNT_HEADER = "#CHR\tPOS\tCount_A\tCount_C\tCount_G\tCount_T\tGood_depth\n"


def digest(files):
    h = hashlib.sha256()
    for k in sorted(files):
        h.update(k.encode())
        h.update(files[k].encode())
    return h.hexdigest()


def _count_row(ctg, pos, counts):
    return "%s\t%d\t%d\t%d\t%d\t%d\t%d\n" % (ctg, pos, counts[0], counts[1], counts[2], counts[3], sum(counts))


def count_files(spec):
    """spec: dict(seed, contigs=[names with files], contig_fn=[names listed], rows=per contig) -> {file name: text}"""
    rng = random.Random(spec["seed"])
    files = {"contigs.txt": "".join(c + "\n" for c in spec["contig_fn"])}
    for ci, ctg in enumerate(spec["contigs"]):
        positions = sorted(rng.sample(range(1000, 900000), spec["rows"]))
        alleles, tumor, normal = ["position\ta0\ta1\n"], [COUNT_HEADER], [COUNT_HEADER]
        for i, pos in enumerate(positions):
            a0, a1 = (i + ci) % 4, ((i + ci) // 4) % 4                     # every ordered pair, equal letters included
            if i % 11 != 5:                                                # the others are loci the allele file does not have
                alleles.append("%d\t%d\t%d\n" % (pos, a0 + 1, a1 + 1))
            if i == 20:
                alleles.append("%d\t%d\t%d\n" % (pos, (a0 + 1) % 4 + 1, (a1 + 2) % 4 + 1))      # the position again: the last row counts
            depth = rng.randint(200, 400)
            t = [rng.randint(0, 3) for _ in range(4)]
            n = [rng.randint(0, 2) for _ in range(4)]
            if i % 13 == 7:                                                # zero-total tumour row: only the two other letters are seen
                t[a0] = t[a1] = 0
                t[[k for k in range(4) if k not in (a0, a1)][0]] += 5
            else:
                alt = sum(rng.random() < (0.5 if i % 3 else 0.01) for _ in range(depth))
                t[a0] += depth - alt
                t[a1] += alt
            if i % 7 == 3:                                                 # normal totals on both sides of 10
                n = [0, 0, 0, 0]
                total = (8, 9, 10, 11)[(i // 7) % 4]
                if a0 == a1:
                    total -= total % 2                                     # (the one letter is counted as ref and as alt)
                    n[a0] = total // 2
                else:
                    n[a0], n[a1] = total - total // 3, total // 3
            else:
                d = rng.randint(15, 60)
                alt = sum(rng.random() < 0.5 for _ in range(d))
                n[a0] += d - alt
                n[a1] += alt
            if i % 17 != 9:                                                # a locus the tumour table lacks
                tumor.append(_count_row(ctg, pos, t))
            if i % 19 != 4:                                                # and one the normal table lacks
                normal.append(_count_row(ctg, pos, n))
            if i == 30:                                                    # a repeated position: first place, last value
                tumor.append(_count_row(ctg, pos, [c + 7 for c in t]))
                normal.append(_count_row(ctg, pos, [c + 4 for c in n]))
        files["alleles_%s.txt" % ctg] = "".join(alleles)
        files["tumor_%s.txt" % ctg] = "".join(tumor)
        files["normal_%s.txt" % ctg] = "".join(normal)
    return files


def rows_for(undecided, proportion_homo=0.65):
    """the n nearest undecided / (1 - proportion_homo) with round(n * proportion_homo) == n - undecided"""
    n0 = round(undecided / (1 - proportion_homo))
    for d in range(0, 50):
        for n in (n0 + d, n0 - d):
            if n > undecided and round(n * proportion_homo) == n - undecided:
                return n
    raise ValueError("no row count for %d undecided probes" % undecided)


def baf_files(spec):
    """spec: dict(seed, runs=[(chromosome name, undecided probes)]) -> {"baf.txt", "logr.txt", "normal_baf.txt"}"""
    rng = random.Random(spec["seed"])
    undecided = sum(m for _, m in spec["runs"])
    n = rows_for(undecided)
    homo = [(n - undecided) // len(spec["runs"])] * len(spec["runs"])
    homo[-1] += n - undecided - sum(homo)
    baf, logr, normal = ["Chromosome\tPosition\tS\n"], ["Chromosome\tPosition\tS\n"], ["Chromosome\tPosition\tN\n"]
    pos = 0
    for (ctg, m), h in zip(spec["runs"], homo):
        kinds = [1] * m + [0] * h
        rng.shuffle(kinds)
        for het in kinds:
            pos += rng.randint(50, 5000)
            depth = rng.randint(200, 400)
            if het:
                alt = sum(rng.random() < 0.5 for _ in range(depth))
                alt = min(max(alt, depth // 4), depth - depth // 4)        # far from the homozygous values
            else:
                alt = rng.choice((0, 1, 2, depth - 2, depth - 1, depth))
            baf.append("%s\t%d\t%s\n" % (ctg, pos, str(alt / depth)))
            logr.append("%s\t%d\t%s\n" % (ctg, pos, str(rng.gauss(0, 0.3))))
            nv = rng.choice((0.0, 0.3, 0.7, 1.0, 0.29999, 0.70001)) if rng.random() < 0.1 else rng.random()
            normal.append("%s\t%d\t%s\n" % (ctg, pos, str(nv)))
    return {"baf.txt": "".join(baf), "logr.txt": "".join(logr), "normal_baf.txt": "".join(normal)}
