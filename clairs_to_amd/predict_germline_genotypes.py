"""Step 4 of the Verdict chain (src/verdict/predict_germline_genotypes.py of the reference, run by src/cna_germline_tagging.py:116-127):
a BAF table -> Tumor_GG.txt, one homozygous (True) / heterozygous (False) flag per locus.

    python -m clairs_to_amd predict_germline_genotypes --tumor_logr_file F --tumor_baf_file F --germline_genotypes_output_file F
           [--normal_baf_file F] [--maxHomozygous 0.02] [--proportionHetero 0.3] [--proportionHomo 0.65] [--proportionOpen 0.03]
           [--segmentLength 100] [--sample_name S] [--where device|host]

With a normal BAF file the flag is baf < 0.3 or baf > 0.7 of the normal (:191-192).  Without one, the probes whose mirrored BAF lies
under homoLimit are homozygous; of the rest, the extraHetero probes closest to one of three window medians of their undecided neighbours
become heterozygous.  Those distances are cto_germline_window_dist (csrc/germline.hip: the rules, the kernel, the host path); everything
that decides a printed byte - the quantile, the two rounds, numpy's argsort of the distances - happens here, on the host, as the
reference does it.  Deviation: --segmentLength below 2 is refused (the reference dies with int(nan) once a run has more than five
undecided probes); a BAF that is not a number is an error of the C call."""
import argparse
import ctypes as C
import sys

import numpy as np

GG_TILE = 64                 # CTO_GG_TILE of include/clairsto_amd.h: probes of one run per workgroup
GG_MAX_SEGMENT = 256         # CTO_GG_MAX_SEGMENT: the largest --segmentLength the kernel takes; above it the C call runs its host code


def _default_where():
    import torch
    return "device" if torch.cuda.is_available() else "host"


def read_table(path):
    """(chr, pos string) -> third column, in file order; a repeated key keeps its first place and its last value (:22-30)"""
    table = {}
    with open(path) as f:
        for i, line in enumerate(f.readlines()):
            if i == 0:
                continue
            c = line.strip().split("\t")
            table[(str(c[0]), str(c[1]))] = c[2]
    return table


def window_dist(c, run_off, segment_length, where="device", stats=None):
    """fp64 distances of cto_germline_window_dist for the concatenated runs `c` (fp64) with offsets `run_off` (n_runs + 1).
    where: "device" (the kernel; above CTO_GG_MAX_SEGMENT the call itself takes its host path) or "host".  stats: a dict that
    receives the call's cto_germline_stats."""
    from ._lib import GermlineStats, check, lib
    if where not in ("device", "host"):
        raise ValueError("where must be 'device' or 'host'")
    c = np.ascontiguousarray(c, dtype=np.float64)
    run_off = np.ascontiguousarray(run_off, dtype=np.int64)
    if run_off.ndim != 1 or len(run_off) < 1 or c.ndim != 1 or int(run_off[-1]) != len(c):
        raise ValueError("run_off must hold n_runs + 1 offsets ending at len(c)")
    dist = np.empty(len(c), dtype=np.float64)
    st = GermlineStats()
    check(lib.cto_germline_window_dist(c.ctypes.data, run_off.ctypes.data, len(run_off) - 1, int(segment_length), 0 if where == "device" else 1,
                                       dist.ctypes.data, C.byref(st)))
    if stats is not None:
        for name, _ in GermlineStats._fields_:
            stats[name] = getattr(st, name)
    return dist


def undecided_runs(chroms, undecided):
    """Offsets (n_runs + 1) into the undecided probes, one run per stretch of equal chromosome names in file order (:32-47); a name that
    comes back later starts a new run."""
    chroms = np.asarray(chroms, dtype=object)
    starts = np.nonzero(np.concatenate(([True], chroms[1:] != chroms[:-1])))[0] if len(chroms) else np.zeros(0, dtype=np.int64)
    before = np.concatenate(([0], np.cumsum(undecided, dtype=np.int64)))          # undecided probes before probe i
    return np.concatenate((before[starts], [before[-1]])).astype(np.int64)


def tumour_only_genotypes(bafs, chroms, max_homozygous, proportion_hetero, proportion_homo, proportion_open, segment_length, where, stats=None):
    """bool array, True = homozygous (:49-166)"""
    tbsam = np.array(bafs).astype(float)
    n = len(tbsam)
    bsm = np.where(tbsam < 0.5, tbsam, 1 - tbsam)
    homo_limit = max(np.sort(bsm)[round(n * proportion_homo)], max_homozygous)     # an index past the end raises, as in the reference
    hom = bsm < homo_limit
    undecided = ~hom
    n_undecided = np.sum(undecided)
    extra_hetero = round(min(proportion_hetero * n, n_undecided - proportion_open * n))
    if extra_hetero <= 0:
        return np.ones(n, dtype=bool)
    probes = np.nonzero(undecided)[0]
    run_off = undecided_runs(chroms, undecided)
    if (np.diff(run_off) <= 5).all():
        dist = np.ones(len(probes), dtype=np.int64)             # the reference's list holds Python ints only: argsort of an integer array
    else:
        dist = window_dist(bsm[probes], run_off, segment_length, where, stats)
    order = np.argsort(dist)                                    # numpy's default kind, on the host: its choice among equal distances
    hom = np.ones(n, dtype=bool)
    hom[probes[order[:min(len(dist), extra_hetero)]]] = False
    return hom


def predict_germline_genotypes(tumor_logr_file, tumor_baf_file, normal_baf_file, output_file, max_homozygous=0.02, proportion_hetero=0.30,
                               proportion_homo=0.65, proportion_open=0.03, segment_length=100, sample_name="SAMPLE", where=None, stats=None):
    if normal_baf_file is None:
        if segment_length < 2:
            sys.exit("predict_germline_genotypes: --segmentLength must be at least 2 (the reference fails on int(nan) below that)")
        open(tumor_logr_file).close()                           # opened as the reference does (a missing file fails); no value of it is used
        table = read_table(tumor_baf_file)
        hom = tumour_only_genotypes(list(table.values()), [k[0] for k in table], max_homozygous, proportion_hetero, proportion_homo,
                                    proportion_open, segment_length, where or _default_where(), stats)
    else:
        table = read_table(normal_baf_file)
        baf = np.array(list(table.values()), dtype=float)
        hom = (baf < 0.3) | (baf > 0.7)
    with open(output_file, "w") as f:
        f.write("Chromosome\tPosition\t%s\n" % sample_name)
        for (ctg, pos), h in zip(table, hom):
            f.write("%s\t%s\t%s\n" % (ctg, pos, "True" if h else "False"))


def main(argv=None):
    ap = argparse.ArgumentParser(prog="predict_germline_genotypes", description="Predict Germline Genotypes")
    ap.add_argument("--tumor_logr_file", type=str, default=None)
    ap.add_argument("--tumor_baf_file", type=str, default=None)
    ap.add_argument("--normal_baf_file", type=str, default=None)
    ap.add_argument("--germline_genotypes_output_file", type=str, default=None)
    ap.add_argument("--maxHomozygous", type=float, default=0.02)
    ap.add_argument("--proportionHetero", type=float, default=0.30)
    ap.add_argument("--proportionHomo", type=float, default=0.65)
    ap.add_argument("--proportionOpen", type=float, default=0.03)
    ap.add_argument("--segmentLength", type=int, default=100)
    ap.add_argument("--sample_name", type=str, default="SAMPLE")
    ap.add_argument("--where", choices=("device", "host"), default=None, help="ours: where the window distances run; default: device when a GPU is present")
    a = ap.parse_args(argv)
    predict_germline_genotypes(a.tumor_logr_file, a.tumor_baf_file, a.normal_baf_file, a.germline_genotypes_output_file, a.maxHomozygous,
                               a.proportionHetero, a.proportionHomo, a.proportionOpen, a.segmentLength, a.sample_name, a.where)
    return 0


if __name__ == "__main__":
    main(sys.argv[1:])
