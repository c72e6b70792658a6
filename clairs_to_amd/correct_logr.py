"""Step 3 of the Verdict chain (src/verdict/correct_logr.py of the reference, run by src/cna_germline_tagging.py:167-197): the tumour logR,
corrected for GC content and replication timing -> the logR table that predict_germline_genotypes opens and aspcf and run_ascat use.

    python -m clairs_to_amd correct_logr --tumor_logr_file F --gc_content_file F --replication_timing_file F
           --tumor_logr_correction_output_file F [--sample_name S] [--where device|host]

The arithmetic over every probe is one cto_correct_logr call (csrc/correctlogr.hip: the rules, the kernels, the host path): the column
statistics of both annotation tables, the B-spline design of the three chosen columns, its least-squares fit and the residuals.  What
stays here is what decides a printed byte without arithmetic: the three tables as dicts in the reference's order (a repeated key keeps its
first place and its last value; the rows follow the logR table), the three np.argmax calls on the correlations the call returns (the
first NaN wins, the windows follow Python's slice rules, and the results index the table one column off from what was correlated - all
as in the reference), and the str() of every residual.  scipy and scikit-learn are not imported.

Where the reference dies, so do we, with a message: a logR key that an annotation table lacks (KeyError there), fewer than 8 GC columns
(ValueError there), a chosen column that is constant (NaN in the regression there).  The residuals are the reference's up to rounding:
they are the projection of the logR off the design's column space, which does not depend on how the rank-deficient system is solved
(DESIGN.md "logR correction")."""
import argparse
import ctypes as C
import sys

import numpy as np

from .predict_germline_genotypes import read_table

BLOCK_ROWS = 256             # CTO_CORRECT_LOGR_BLOCK_ROWS of include/clairsto_amd.h: the rows of one block of the fixed summation tree

INDEX_1KB = 5
INDEX_MAX = 11


def _default_where():
    import torch
    return "device" if torch.cuda.is_available() else "host"


# ------------------------------------------------------------------------------------------------ the C calls
def fit(logr, gc, rt, where="device", stats=None):
    """(corr_gc, corr_rt, residual) of cto_correct_logr for logr (N), gc (N x G) and rt (N x T).  where: "device" or "host".
    stats: a dict that receives the call's cto_correct_logr_stats."""
    from ._lib import CorrectLogrStats, check, lib
    if where not in ("device", "host"):
        raise ValueError("where must be 'device' or 'host'")
    logr, gc, rt = [np.ascontiguousarray(v, dtype=np.float64) for v in (logr, gc, rt)]
    if logr.ndim != 1 or gc.ndim != 2 or rt.ndim != 2 or gc.shape[0] != len(logr) or rt.shape[0] != len(logr):
        raise ValueError("logr must be flat, gc and rt tables with one row per logR value")
    corr_gc, corr_rt, residual = np.zeros(gc.shape[1]), np.zeros(rt.shape[1]), np.zeros(len(logr))
    st = CorrectLogrStats()
    rc = lib.cto_correct_logr(logr.ctypes.data, len(logr), gc.ctypes.data, gc.shape[1], rt.ctypes.data, rt.shape[1], 0 if where == "device" else 1,
                              corr_gc.ctypes.data, corr_rt.ctypes.data, residual.ctypes.data, C.byref(st))
    if stats is not None:
        for name, _ in CorrectLogrStats._fields_:
            stats[name] = getattr(st, name)
    check(rc)
    return corr_gc, corr_rt, residual


def bspline_basis(x, lo, hi):
    """the five cubic B-splines of create_bspline_basis(., df=5) at every x, for a column whose minimum is lo and maximum hi
    (cto_correct_logr_basis): len(x) x 5"""
    from ._lib import check, lib
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.zeros((len(x), 5))
    check(lib.cto_correct_logr_basis(x.ctypes.data, len(x), float(lo), float(hi), out.ctypes.data))
    return out


# ------------------------------------------------------------------------------------------------ the tables
def read_annotation(path):
    """('chr' + second field, third field) -> the fields behind them, in file order; a repeated key keeps its first place and its last
    value (:33-50)"""
    table = {}
    with open(path) as f:
        for i, line in enumerate(f.readlines()):
            if i == 0:
                continue
            c = line.strip().split("\t")
            table[("chr" + str(c[1]), str(c[2]))] = c[3:]
    return table


def rows_of(table, keys, what):
    try:
        return np.array([table[key] for key in keys]).astype(float)
    except KeyError as e:
        sys.exit("correct_logr: the %s table has no row for %r, a locus of the logR table (the reference fails there, on a KeyError)" % (what, e.args[0]))


def chosen_columns(corr_gc, corr_rt):
    """(maxGCcol_insert, maxGCcol_amplic, maxreplic) of :62-74"""
    return (int(np.argmax(corr_gc[:(INDEX_1KB + 1)])), int(np.argmax(corr_gc[(INDEX_1KB + 2):(INDEX_MAX + 1)]) + (INDEX_1KB + 2)),
            int(np.argmax(corr_rt)))


def correct_logr(tumor_logr_file, gc_content_file, replication_timing_file, tumor_logr_correction_output_file, sample_name="SAMPLE", where=None,
                 stats=None):
    logr_table = read_table(tumor_logr_file)
    gc_table, rt_table = read_annotation(gc_content_file), read_annotation(replication_timing_file)
    keys = list(logr_table.keys())
    logr = np.array(list(logr_table.values())).astype(float)
    gc, rt = rows_of(gc_table, keys, "GC content"), rows_of(rt_table, keys, "replication timing")
    if gc.ndim != 2 or gc.shape[1] < INDEX_1KB + 3:
        sys.exit("correct_logr: the GC content table has %s value columns, fewer than the %d the second window needs (the reference fails "
                 "there, on the argmax of an empty window)" % (gc.shape[1] if gc.ndim == 2 else "ragged", INDEX_1KB + 3))
    st = {}
    corr_gc, corr_rt, residual = fit(logr, gc, rt, where or _default_where(), st)
    if stats is not None:
        stats.update(st)
    cols = chosen_columns(corr_gc, corr_rt)
    if cols != (st["col_insert"], st["col_amplic"], st["col_replic"]):
        sys.exit("correct_logr: the fit used columns %r where np.argmax chooses %r" % ((st["col_insert"], st["col_amplic"], st["col_replic"]), cols))
    with open(tumor_logr_correction_output_file, "w") as f:
        f.write("Chromosome\tPosition\t" + sample_name + "\n")
        f.writelines("\t".join(map(str, key)) + "\t" + str(value) + "\n" for key, value in zip(keys, residual))


def main(argv=None):
    ap = argparse.ArgumentParser(prog="correct_logr", description="Correct Tumor Sample LogR")
    ap.add_argument('--tumor_logr_file', type=str, default=None, help="Path of tumor sample LogR")
    ap.add_argument('--gc_content_file', type=str, default=None, help="Path of 1kG GC content file")
    ap.add_argument('--replication_timing_file', type=str, default=None, help="Path of 1kG replication timing file")
    ap.add_argument('--tumor_logr_correction_output_file', type=str, default=None, help="Output path of tumor sample corrected LogR")
    ap.add_argument('--sample_name', type=str, default="SAMPLE", help="Tumor sample name")
    ap.add_argument("--where", choices=("device", "host"), default=None, help="ours: where the fit is computed; default: device when a GPU is present")
    a = ap.parse_args(argv)
    correct_logr(a.tumor_logr_file, a.gc_content_file, a.replication_timing_file, a.tumor_logr_correction_output_file, a.sample_name, a.where)
    return 0


if __name__ == "__main__":
    main(sys.argv[1:])
