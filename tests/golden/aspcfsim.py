"""Synthetic inputs of the Verdict step aspcf (src/verdict/aspcf.py of the reference): a logR table, a BAF table and a germline genotype
table with the same keys, laid out so that every run of chromosome names holds the spec's number of heterozygous probes.  Input synthesis
for gen_aspcf.py and for the tests, which regenerate the inputs from the specs and check them against the stored SHA-256.  The product
never imports this.

tables(spec): spec = dict(seed, chroms=[(name, heterozygous probes, heterozygous probes per level)], hom_per_het, stretch).  A run
holds int(het * hom_per_het) + 30 homozygous probes shuffled among the heterozygous ones.  The logR level (uniform in -0.8 .. 0.8) and
the BAF imbalance (0 .. 0.3 from 0.5, a side drawn per probe) change every `per level` heterozygous probes, give or take a fifth;
noise is Gaussian, 0.12 and 0.03.  Homozygous BAFs are at most 0.008 from 0 or 1.  stretch = (index of the run, probes, shift) or None
puts that many homozygous probes in a row in the middle of the run, their logR shifted."""
import hashlib
import random


def digest(files):
    h = hashlib.sha256()
    for k in sorted(files):
        h.update(k.encode())
        h.update(files[k].encode())
    return h.hexdigest()


def tables(spec):
    rng = random.Random(spec["seed"])
    logr, baf, gg = ["Chromosome\tPosition\tS\n"], ["Chromosome\tPosition\tS\n"], ["Chromosome\tPosition\tS\n"]
    pos = 0
    for ci, (ctg, n_het, per_level) in enumerate(spec["chroms"]):
        kinds = [1] * n_het + [0] * (int(n_het * spec["hom_per_het"]) + 30)
        rng.shuffle(kinds)
        shift_at = {}
        if spec.get("stretch") and spec["stretch"][0] == ci:
            _, length, shift = spec["stretch"]
            mid = len(kinds) // 2
            kinds[mid:mid] = [0] * length
            shift_at = {i: shift for i in range(mid, mid + length)}
        level, delta, left = 0.0, 0.0, 0
        for i, het in enumerate(kinds):
            if het:
                if left == 0:
                    level, delta = rng.uniform(-0.8, 0.8), rng.uniform(0.0, 0.3)
                    left = max(1, per_level + rng.randint(-(per_level // 5), per_level // 5))
                left -= 1
            pos += rng.randint(50, 5000)
            lr = level + shift_at.get(i, 0.0) + rng.gauss(0, 0.12)
            if het:
                b = min(max(0.5 + rng.choice((-1, 1)) * delta + rng.gauss(0, 0.03), 0.05), 0.95)
            else:
                b = rng.choice((0.0, 0.004, 0.008, 0.992, 0.996, 1.0))
            logr.append("%s\t%d\t%s\n" % (ctg, pos, str(lr)))
            baf.append("%s\t%d\t%s\n" % (ctg, pos, str(b)))
            gg.append("%s\t%d\t%s\n" % (ctg, pos, "False" if het else "True"))
    return {"logr.txt": "".join(logr), "baf.txt": "".join(baf), "gg.txt": "".join(gg)}
