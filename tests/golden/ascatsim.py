"""Synthetic inputs of the Verdict step run_ascat (src/verdict/run_ascat.py of the reference): the logR, BAF and germline genotype tables
and the two segmented tables that aspcf would write for them (the segmented logR of every probe, the segmented BAF of every heterozygous
probe), all with the same keys.  Input synthesis for gen_ascat.py and for the tests, which regenerate the inputs from the specs and check
them against the stored SHA-256.  The product never imports this.

tables(spec): spec = dict(seed, purity, ploidy, gamma, states=[(nMajor, nMinor, weight)], chroms=[(name, segments)], het=(lo, hi),
hom_per_het, noise=(sd of a logR level, sd of a BAF level), hom_runs=[segment numbers], hom_run=(rows, shift)).  Every segment draws a
state and lo .. hi heterozygous probes, with int(het * hom_per_het) + 5 homozygous probes shuffled among them.  Its tracks are piecewise
constant: one logR level gamma * log2((2 (1 - rho) + rho (nMajor + nMinor)) / (2 (1 - rho) + rho ploidy)) and one BAF level
(1 - rho + rho nMinor) / (2 - 2 rho + rho (nMajor + nMinor)), each with one draw of noise per segment and then repeated without noise
over the segment's probes; a balanced state has the BAF level 0.5 exactly, as aspcf writes it.  A segment named in hom_runs gets that
many homozygous probes in a row in its middle, their segmented logR shifted: a run of equal logR without a heterozygous probe inside.
The raw BAF of a heterozygous probe lies on either side of 0.5, that of a homozygous probe at most 0.008 from 0 or 1."""
import hashlib
import math
import random

FILES = ("logr.txt", "baf.txt", "gg.txt", "seg_logr.txt", "seg_baf.txt")


def digest(files):
    h = hashlib.sha256()
    for k in sorted(files):
        h.update(k.encode())
        h.update(files[k].encode())
    return h.hexdigest()


def tables(spec):
    rng = random.Random(spec["seed"])
    rho, psi, gamma = spec["purity"], spec["ploidy"], spec["gamma"]
    base = 2 * (1 - rho) + rho * psi
    states = [(a, b) for a, b, _ in spec["states"]]
    weights = [w for _, _, w in spec["states"]]
    head = "Chromosome\tPosition\tS\n"
    out = {k: [head] for k in FILES}
    pos, seg_no = 0, 0
    for ctg, n_seg in spec["chroms"]:
        for _ in range(n_seg):
            major, minor = rng.choices(states, weights)[0]
            n_het = rng.randint(*spec["het"])
            kinds = [1] * n_het + [0] * (int(n_het * spec["hom_per_het"]) + 5)
            rng.shuffle(kinds)
            shifted = {}
            if seg_no in spec["hom_runs"]:
                rows, shift = spec["hom_run"]
                mid = len(kinds) // 2
                kinds[mid:mid] = [0] * rows
                shifted = {i: shift for i in range(mid, mid + rows)}
            total = 2 * (1 - rho) + rho * (major + minor)
            level = gamma * math.log2(total / base) + rng.gauss(0, spec["noise"][0])
            b = 0.5 if major == minor else min(max((1 - rho + rho * minor) / total + rng.gauss(0, spec["noise"][1]), 0.001), 0.499)
            for i, het in enumerate(kinds):
                pos += rng.randint(50, 5000)
                key = "%s\t%d\t" % (ctg, pos)
                raw_b = min(max(rng.choice((b, 1 - b)) + rng.gauss(0, 0.03), 0.02), 0.98) if het else rng.choice((0.0, 0.004, 0.008, 0.992, 0.996, 1.0))
                out["logr.txt"].append(key + str(level + rng.gauss(0, 0.1)) + "\n")
                out["baf.txt"].append(key + str(raw_b) + "\n")
                out["gg.txt"].append(key + ("False" if het else "True") + "\n")
                out["seg_logr.txt"].append(key + str(level + shifted.get(i, 0.0)) + "\n")
                if het:
                    out["seg_baf.txt"].append(key + str(b) + "\n")
            seg_no += 1
    return {k: "".join(v) for k, v in out.items()}
