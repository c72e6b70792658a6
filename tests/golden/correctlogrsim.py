"""Synthetic inputs of the Verdict step correct_logr (src/verdict/correct_logr.py of the reference): the tumour logR table and the two
annotation tables it is corrected with, GC content and replication timing.  Input synthesis for gen_correct_logr.py and for the tests,
which regenerate the inputs from the specs and check them against the stored SHA-256.  The product never imports this.

tables(spec): spec = dict(seed, chroms=[(name, probes)], G, T, extra, shuffle, repeats, constant_gc, missing).  Every probe draws a latent
GC fraction (skewed: a beta distribution) and a latent replication timing; GC column j is the latent fraction seen through a window of
its own (a mix with an independent draw, the mix drawn once per column) and RT column j the latent timing with noise of a width of its
own, so which columns the argmax rules choose differs from seed to seed; the logR is a smooth function of both plus noise.  Annotation
rows are `id \t chromosome without "chr" \t position \t values`, as the reference reads them; values are printed with six decimals.
  * extra: so many annotation rows for loci that the logR table lacks, in each annotation file;
  * shuffle: the annotation rows in an order of their own (each file its own);
  * repeats: so many keys written twice in each of the three files, the second time with other values (the reference keeps the first
    place and the last value);
  * constant_gc: a GC column whose every value is 0.25, or None;
  * missing: so many logR keys that the GC file lacks (the last probes of the table)."""
import hashlib
import math
import random

FILES = ("logr.txt", "gc.txt", "rt.txt")


def digest(files):
    h = hashlib.sha256()
    for k in sorted(files):
        h.update(k.encode())
        h.update(files[k].encode())
    return h.hexdigest()


def annotation_row(rng, mixes, widths, constant_gc):
    g, t = rng.betavariate(4.0, 6.0), rng.gauss(0.0, 1.0)
    gc = [min(max((1 - mix) * g + mix * rng.betavariate(4.0, 6.0) + rng.gauss(0, 0.01), 0.0), 1.0) for mix in mixes]
    if constant_gc is not None:
        gc[constant_gc] = 0.25
    rt = [40.0 + 18.0 * t + rng.gauss(0, width) for width in widths]
    return g, t, gc, rt


def line_of(ident, ctg, pos, values):
    return "%s\t%s\t%d\t%s\n" % (ident, ctg[3:], pos, "\t".join("%.6f" % v for v in values))


def tables(spec):
    rng = random.Random(spec["seed"])
    G, T = spec["G"], spec["T"]
    mixes, widths = [rng.uniform(0.08, 0.92) for _ in range(G)], [rng.uniform(4.0, 20.0) for _ in range(T)]
    logr, gc, rt = [], [], []
    pos, n = 0, 0
    for ctg, probes in spec["chroms"]:
        for _ in range(probes):
            pos += rng.randint(50, 5000)
            g, t, gcv, rtv = annotation_row(rng, mixes, widths, spec.get("constant_gc"))
            y = -1.8 * (g - 0.4) + 6.0 * (g - 0.4) ** 2 + 0.06 * t - 0.02 * math.sin(2.0 * t) + rng.gauss(0, 0.12)
            logr.append("%s\t%d\t%s\n" % (ctg, pos, repr(y)))
            gc.append(line_of("snp%d" % n, ctg, pos, gcv))
            rt.append(line_of("snp%d" % n, ctg, pos, rtv))
            n += 1
    for k in range(spec.get("repeats", 0)):                     # the same key again, further down, with other values
        for rows, kind in ((logr, 0), (gc, 1), (rt, 2)):
            at = rng.randrange(len(rows) // 2)
            c = rows[at].split("\t")
            _, _, gcv, rtv = annotation_row(rng, mixes, widths, spec.get("constant_gc"))
            if kind == 0:
                rows.insert(rng.randrange(at + 1, len(rows) + 1), "%s\t%s\t%s\n" % (c[0], c[1], repr(rng.gauss(0, 0.3))))
            else:
                rows.insert(rng.randrange(at + 1, len(rows) + 1), line_of(c[0] + "b", "chr" + c[1], int(c[2]), gcv if kind == 1 else rtv))
    if spec.get("missing", 0):
        del gc[-spec["missing"]:]
    for k in range(spec.get("extra", 0)):                       # loci the logR table lacks
        pos += rng.randint(50, 5000)
        _, _, gcv, rtv = annotation_row(rng, mixes, widths, spec.get("constant_gc"))
        gc.append(line_of("extra%d" % k, "chr21", pos, gcv))
        rt.append(line_of("extra%d" % k, "chr22", pos + 7, rtv))
    if spec.get("shuffle"):
        rng.shuffle(gc)
        rng.shuffle(rt)
    return {"logr.txt": "Chromosome\tPosition\tS\n" + "".join(logr),
            "gc.txt": "\tChr\tPosition\t" + "\t".join("gc%d" % j for j in range(G)) + "\n" + "".join(gc),
            "rt.txt": "\tChr\tPosition\t" + "\t".join("rt%d" % j for j in range(T)) + "\n" + "".join(rt)}
