"""Step 2 of the Verdict chain (src/verdict/get_logr_and_baf.py of the reference, run by src/cna_germline_tagging.py:92-103): the
per-contig allele count tables of allele_counter plus the 1000G allele files -> Tumor_LogR.txt, Tumor_BAF.txt and, with a normal,
Normal_BAF.txt.  Host only: the tables are small, and every printed digit is a Python float's str(), as in the reference.

    python -m clairs_to_amd get_logr_and_baf --tumor_allele_counts_file_prefix P --alleles_file_prefix A --contig_fn CONTIGS
           --tumor_logr_output_file F --tumor_baf_output_file F [--normal_allele_counts_file_prefix P --normal_baf_output_file F]
           [--sample_name S] [--normal_sample_name S] [--seed N]

The reference prints, per kept row, random.choice([ref / total, alt / total]) from a generator it seeds with int(time()) on import.
--seed (ours) draws from random.Random(seed) instead, one choice per kept row in the reference's order (per contig: the tumour rows,
then the normal rows): the BAF files are then the bytes the reference writes when its `random` is re-seeded with the same number."""
import argparse
import math
import random
from time import time

MAJOR_CONTIGS = ["chr%s" % c for c in list(range(1, 23)) + ["X"]]        # :11
ALLELE_OF = {"1": "A", "2": "C", "3": "G", "4": "T"}                     # :15
COLUMN_OF = {"A": 2, "C": 3, "G": 4, "T": 5}                             # of a count row: #CHR POS Count_A Count_C Count_G Count_T Good_depth


def read_contigs(contig_fn):
    with open(contig_fn) as f:
        return [c.strip() for c in f if c.strip() in MAJOR_CONTIGS]


def read_alleles(path, ctg, alleles):
    """(ctg, pos string) -> (ref letter, alt letter); a repeated position keeps its last row (:31-38)"""
    with open(path) as f:
        for i, line in enumerate(f.readlines()):
            if i == 0:
                continue
            c = line.strip().split("\t")
            alleles[(ctg, c[0])] = (ALLELE_OF[c[1]], ALLELE_OF[c[2]])


def read_counts(path, ctg, alleles, dropped, rng, totals, bafs):
    """One count table into totals / bafs (:42-82, :87-127).  The key is the row's own first column; a repeated key keeps its first
    place and its last value; one draw per kept row."""
    with open(path) as f:
        for i, line in enumerate(f.readlines()):
            if i == 0:
                continue
            c = line.strip().split("\t")
            pair = alleles.get((ctg, c[1]))
            if pair is None:
                continue
            n_ref, n_alt = int(c[COLUMN_OF[pair[0]]]), int(c[COLUMN_OF[pair[1]]])
            total = n_ref + n_alt
            if dropped(total):
                continue
            key = (c[0], c[1])
            totals[key] = total
            bafs[key] = rng.choice([n_ref / total, n_alt / total])


def get_bafs_and_logrs(tumor_prefix, normal_prefix, alleles_prefix, contigs, rng):
    """(logR, tumour BAF, normal BAF or None): dicts keyed by (chr, pos string) in output order"""
    alleles, t_tot, t_baf, n_tot, n_baf = {}, {}, {}, {}, {}
    for ctg in contigs:
        read_alleles("%s%s.txt" % (alleles_prefix, ctg), ctg, alleles)
        read_counts("%s%s.txt" % (tumor_prefix, ctg), ctg, alleles, lambda t: t == 0, rng, t_tot, t_baf)       # :77
        if normal_prefix is not None:
            read_counts("%s%s.txt" % (normal_prefix, ctg), ctg, alleles, lambda t: t < 10, rng, n_tot, n_baf)  # :122
    if normal_prefix is None:
        mean_t = sum(t_tot.values()) / len(t_tot)
        return {k: math.log2(v / mean_t) for k, v in t_tot.items()}, t_baf, None
    common = [k for k in t_tot if k in n_tot]
    mean_t = sum(t_tot[k] for k in common) / len(common)
    mean_n = sum(n_tot[k] for k in common) / len(common)
    logr = {k: math.log2((t_tot[k] / mean_t) / (n_tot[k] / mean_n)) for k in common}
    return logr, {k: t_baf[k] for k in common}, {k: n_baf[k] for k in common}


def write_table(path, sample_name, table):
    with open(path, "w") as f:
        f.write("Chromosome\tPosition\t%s\n" % sample_name)
        for (ctg, pos), v in table.items():
            f.write("%s\t%s\t%s\n" % (ctg, pos, str(v)))


def main(argv=None):
    ap = argparse.ArgumentParser(prog="get_logr_and_baf", description="Get Sample LogR and BAF")
    ap.add_argument("--tumor_allele_counts_file_prefix", type=str, default=None)
    ap.add_argument("--normal_allele_counts_file_prefix", type=str, default=None)
    ap.add_argument("--alleles_file_prefix", type=str, default=None)
    ap.add_argument("--tumor_logr_output_file", type=str, default=None)
    ap.add_argument("--tumor_baf_output_file", type=str, default=None)
    ap.add_argument("--normal_baf_output_file", type=str, default=None)
    ap.add_argument("--sample_name", type=str, default="SAMPLE")
    ap.add_argument("--normal_sample_name", type=str, default="NORMAL_SAMPLE")
    ap.add_argument("--contig_fn", type=str, default=None)
    ap.add_argument("--seed", type=int, default=None, help="seed of the BAF draws (ours; default int(time()), as the reference seeds on import)")
    a = ap.parse_args(argv)
    rng = random.Random(int(time()) if a.seed is None else a.seed)
    logr, t_baf, n_baf = get_bafs_and_logrs(a.tumor_allele_counts_file_prefix, a.normal_allele_counts_file_prefix, a.alleles_file_prefix,
                                            read_contigs(a.contig_fn), rng)
    write_table(a.tumor_logr_output_file, a.sample_name, logr)
    write_table(a.tumor_baf_output_file, a.sample_name, t_baf)
    if n_baf is not None:
        write_table(a.normal_baf_output_file, a.normal_sample_name, n_baf)
    return 0


if __name__ == "__main__":
    import sys
    main(sys.argv[1:])
