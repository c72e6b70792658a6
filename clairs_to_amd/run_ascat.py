"""Step 6 of the Verdict chain (src/verdict/run_ascat.py of the reference, run by src/cna_germline_tagging.py:143-164): the segmented logR
and BAF of aspcf -> the tumour's purity, ploidy and goodness of fit, and its allele-specific copy-number segments.

    python -m clairs_to_amd run_ascat --tumor_logr_file F --tumor_baf_file F --germline_genotypes_file F --tumor_logr_segmented_file F
           --tumor_baf_segmented_file F --tumor_purity_ploidy_output_file F --tumor_cna_output_file F [--gamma 1.0] [--min_ploidy 1.5]
           [--max_ploidy 5.5] [--min_purity 0.1] [--max_purity 1.05] [--sample_name S] [--where device|host]

The hot path is create_distance_matrix: every cell of the ploidy x purity grid (100 x 95 with the default bounds), three np.nansum over
all segments each.  Here the grid is one cto_ascat_distance call (csrc/ascat.hip: the rules, the kernel, the host path); the power
2 ** (logR / gamma) depends on the segment alone and is taken by numpy, here, in the reference's operand order.  Everything else that
decides a printed byte is numpy on the host in the reference's own operation order: make_segments, the four local-minimum scans (which
overwrite the matrix while they read it, and index grids that are not the ones the matrix was computed on - both kept), the choice of the
first optimum equal to the minimum, the copy numbers per run of equal logR, the 20 merge rounds, the mean that is the ploidy, the str()
of every number.  scipy is not imported.

As in the reference: the tables are matched by row order; when no probe is heterozygous nothing is written; when no scan finds an
optimum a message is printed and nothing is written.  Where the reference dies, so do we, with a message: a run of equal logR with no
heterozygous probe within 10000 rows (it takes the first of an empty array), and bounds that make the matrix larger or smaller than the
grids the scans index (IndexError there)."""
import argparse
import ctypes as C
import sys

import numpy as np

from .predict_germline_genotypes import read_table

LDS_SEGMENTS = 2048          # CTO_ASCAT_LDS_SEGMENTS of include/clairsto_amd.h: above it the kernel reads the segments from global memory

MINABB = 0.03
MINABBREGION = 0.005
MINRHO = 0.2
MINGOODNESSOFFIT = 60
MINPERCZERO = 0.02
MINPERCZEROABB = 0.1
MINPERCODDEVEN = 0.05
MINPLOIDYSTRICT = 1.7
MAXPLOIDYSTRICT = 2.3


def _default_where():
    import torch
    return "device" if torch.cuda.is_available() else "host"


# ------------------------------------------------------------------------------------------------ the C call
def distance_matrix(u, w, cnt, wgt, psi, rho, where="device", stats=None):
    """d of cto_ascat_distance, len(psi) x len(rho).  where: "device" or "host".  stats: a dict that receives the call's cto_ascat_stats."""
    from ._lib import AscatStats, check, lib
    if where not in ("device", "host"):
        raise ValueError("where must be 'device' or 'host'")
    u, w, cnt, wgt, psi, rho = [np.ascontiguousarray(v, dtype=np.float64) for v in (u, w, cnt, wgt, psi, rho)]
    if u.ndim != 1 or not (u.shape == w.shape == cnt.shape == wgt.shape) or psi.ndim != 1 or rho.ndim != 1:
        raise ValueError("u, w, cnt and wgt must be flat and of one length, psi and rho flat")
    d = np.zeros((len(psi), len(rho)))
    st = AscatStats()
    check(lib.cto_ascat_distance(u.ctypes.data, w.ctypes.data, cnt.ctypes.data, wgt.ctypes.data, len(u), psi.ctypes.data, len(psi), rho.ctypes.data,
                                 len(rho), 0 if where == "device" else 1, d.ctypes.data, C.byref(st)))
    if stats is not None:
        for name, _ in AscatStats._fields_:
            stats[name] = getattr(st, name)
    return d


def nansum(x):
    """np.nansum of a flat float64 array as cto_ascat_distance takes it (cto_ascat_sum)"""
    from ._lib import check, lib
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = C.c_double(0.0)
    check(lib.cto_ascat_sum(x.ctypes.data, len(x), C.byref(out)))
    return out.value


# ------------------------------------------------------------------------------------------------ numpy, in the reference's order
def make_segments(r, b):
    """(logR, BAF, probes) per run of heterozygous probes with equal logR and equal BAF"""
    m = np.column_stack((r, b))
    segments, previousb, previousr, count = [], -1, 1E10, 0
    for i in range(m.shape[0]):
        if m[i, 1] != previousb or m[i, 0] != previousr:
            if count > 0:
                segments[-1][-1] = count
            count = 1
            segments.append([m[i, 0], m[i, 1], count])
        else:
            count += 1
        previousb = m[i, 1]
        previousr = m[i, 0]
    if count > 0:
        segments[-1][-1] = count
    return np.array(segments, dtype=float)


def grid(min_ploidy=None, max_ploidy=None, min_purity=None, max_purity=None):
    """(psi_pos, rho_pos) of create_distance_matrix"""
    if min_ploidy is None or max_ploidy is None:
        psi_pos = np.arange(1, 6.05, 0.05)
    else:
        psi_pos = np.arange(min_ploidy - 0.5, max_ploidy + 0.5, 0.05)
    if min_purity is None or max_purity is None:
        rho_pos = np.arange(0.1, 1.06, 0.01)
    else:
        rho_pos = np.arange(round(min_purity, 2), round(max_purity, 2), 0.01)
    return psi_pos, rho_pos


def segment_terms(s, gamma):
    """what the grid needs of every segment: (u, w, cnt, wgt), the power taken by numpy in the reference's operand order"""
    return (s[:, 1] - 1) * 2 ** (s[:, 0] / gamma), s[:, 1] * 2 ** (s[:, 0] / gamma), s[:, 2], np.where(s[:, 1] == 0.5, 0.05, 1)


def create_distance_matrix(s, gamma, min_ploidy=None, max_ploidy=None, min_purity=None, max_purity=None, where="device", stats=None):
    psi_pos, rho_pos = grid(min_ploidy, max_ploidy, min_purity, max_purity)
    if len(psi_pos) == 0 or len(rho_pos) == 0:
        return np.zeros((len(psi_pos), len(rho_pos)))
    return distance_matrix(*segment_terms(s, gamma), psi_pos, rho_pos, where, stats)


def rle(x):
    n = len(x)
    y = np.array(x[1:] != x[:-1])
    i = np.append(np.where(y), n - 1)
    return {'lengths': np.diff(np.append(-1, i)), 'values': x[i]}


def grid_value(values, k, what, bound):
    if k >= len(values):
        sys.exit("run_ascat: the distance matrix has a local minimum at %s index %d, beyond the %d values the scans index (the reference fails "
                 "there, on an IndexError): --min_%s / --max_%s are too far apart" % (what, k, len(values), bound, bound))
    return values[k]


def scan(d, s, gamma, psi_values, rho_values, accept):
    """one pass over the 7 x 7 windows of d, which it overwrites as the reference does: [m, i, j, ploidy, goodnessOfFit] of every local
    minimum that accept() lets through"""
    found = []
    TheoretMaxdist = np.sum(0.25 * s[:, 2] * np.where(s[:, 1] == 0.5, 0.05, 1))
    for i in range(3, d.shape[0] - 3):
        for j in range(3, d.shape[1] - 3):
            m = d[i, j]
            seld = d[i - 3:i + 4, j - 3:j + 4]
            seld[3, 3] = np.max(seld)
            if np.min(seld) > m:
                psi = grid_value(psi_values, i, "ploidy", "ploidy")
                rho = grid_value(rho_values, j, "purity", "purity")
                nA = (rho - 1 - (s[:, 1] - 1) * 2 ** (s[:, 0] / gamma) * ((1 - rho) * 2 + rho * psi)) / rho
                nB = (rho - 1 + s[:, 1] * 2 ** (s[:, 0] / gamma) * ((1 - rho) * 2 + rho * psi)) / rho
                ploidy = np.sum((nA + nB) * s[:, 2]) / np.sum(s[:, 2])
                percentzero = (np.sum((np.round(nA) == 0) * s[:, 2]) + np.sum((np.round(nB) == 0) * s[:, 2])) / np.sum(s[:, 2])
                percOddEven = np.sum(((np.round(nA) % 2 == 0) & (np.round(nB) % 2 == 1) | (np.round(nA) % 2 == 1) & (np.round(nB) % 2 == 0)) * s[:, 2]) / np.sum(s[:, 2])
                with np.errstate(invalid="ignore", divide="ignore"):
                    perczeroAbb = (np.sum((np.round(nA) == 0) * s[:, 2] * (s[:, 1] != 0.5)) +
                                   np.sum((np.round(nB) == 0) * s[:, 2] * (s[:, 1] != 0.5))) / np.sum(s[:, 2] * (s[:, 1] != 0.5))
                if np.isnan(perczeroAbb):                       # the BAF is a flat line at 0.5
                    perczeroAbb = 0
                goodnessOfFit = (1 - m / TheoretMaxdist) * 100
                if accept(ploidy, rho, goodnessOfFit, percentzero, perczeroAbb, percOddEven):
                    found.append([m, i, j, ploidy, goodnessOfFit])
    return found


def find_optima(d, s, gamma, min_ploidy, max_ploidy, seen=None):
    """the four scans, each only when the ones before found nothing; `seen` receives which one filled the list"""
    psi_values = np.arange(1.05, 6.05, 0.05)
    rho_values = np.round(np.arange(0.11, 1.06, 0.01), 2)
    percentAbb = np.sum(np.where(s[:, 1] == 0.5, 0, 1) * s[:, 2]) / np.sum(s[:, 2])
    maxsegAbb = np.max(np.where(s[:, 1] == 0.5, 0, s[:, 2])) / np.sum(s[:, 2])
    nonaberrant = bool(percentAbb <= MINABB and maxsegAbb <= MINABBREGION)
    strict_allowed = min_ploidy < MAXPLOIDYSTRICT and max_ploidy > MINPLOIDYSTRICT

    def first(ploidy, rho, gof, percentzero, perczeroAbb, percOddEven):
        return not nonaberrant and min_ploidy < ploidy < max_ploidy and rho >= MINRHO and gof > MINGOODNESSOFFIT and percentzero > MINPERCZERO

    def second(ploidy, rho, gof, percentzero, perczeroAbb, percOddEven):
        return MINPLOIDYSTRICT < ploidy < MAXPLOIDYSTRICT and rho >= MINRHO and gof > MINGOODNESSOFFIT and perczeroAbb > MINPERCZEROABB

    def third(ploidy, rho, gof, percentzero, perczeroAbb, percOddEven):
        return (not nonaberrant and min_ploidy < ploidy < max_ploidy and rho >= MINRHO and gof > MINGOODNESSOFFIT and
                (perczeroAbb > MINPERCZEROABB or percentzero > MINPERCZERO or percOddEven > MINPERCODDEVEN))

    def fourth(ploidy, rho, gof, percentzero, perczeroAbb, percOddEven):
        return MINPLOIDYSTRICT < ploidy < MAXPLOIDYSTRICT and rho >= MINRHO and gof > MINGOODNESSOFFIT

    optima, which = scan(d, s, gamma, psi_values, rho_values, first), 1
    if len(optima) == 0 and strict_allowed:
        optima, which = scan(d, s, gamma, psi_values, rho_values, second), 2
    if len(optima) == 0:
        cold = np.where(rho_values > 1)[0]                      # the borders with rho = 1
        if len(cold) and cold[-1] >= d.shape[1]:
            sys.exit("run_ascat: the distance matrix has %d purities, fewer than the %d the scans index (the reference fails there, on an "
                     "IndexError): --min_purity / --max_purity are too close" % (d.shape[1], len(rho_values)))
        d[:, cold] = 1E20
        optima, which = scan(d, s, gamma, psi_values, rho_values, third), 3
    if len(optima) == 0 and strict_allowed:
        optima, which = scan(d, s, gamma, psi_values, rho_values, fourth), 4
    if seen is not None:
        seen["scan"] = which if optima else 0
        seen["optima"] = len(optima)
    return optima, psi_values, rho_values


def copy_number_segments(rho, psi, gamma, b, r_ori, het_indices, n_probes):
    """[first row, last row, nA, nB] per run of equal segmented logR, neighbours with equal copy numbers merged in 20 rounds"""
    diploidprobes = np.full(n_probes, True, dtype=bool)
    tlr2 = rle(r_ori)
    tlrstart = np.cumsum(np.concatenate(([0], tlr2['lengths'])))[:-1]
    tlrend = np.cumsum(tlr2['lengths']) - 1
    tlr = tlr2['values']
    seg = []
    for i in range(len(tlr)):
        logR, start, end = tlr[i], tlrstart[i], tlrend[i]
        baf_slice = np.where((het_indices > start) & (het_indices < end + 1))[0]
        if len(baf_slice) == 0:
            baf_slice = np.where((het_indices > start - 10000) & (het_indices < end + 1 + 10000))[0]
            if len(baf_slice) == 0:
                sys.exit("run_ascat: no heterozygous probe within 10000 rows of the logR run of rows %d-%d (the reference fails there, on the "
                         "first element of an empty array)" % (start, end))
        bafke = b[baf_slice][0]
        nAraw = np.where(diploidprobes[start],
                         (rho - 1 - (bafke - 1) * 2 ** (logR / gamma) * ((1 - rho) * 2 + rho * psi)) / rho,
                         (rho - 1 + ((1 - rho) * 2 + rho * psi) * 2 ** (logR / gamma)) / rho)
        nBraw = np.where(diploidprobes[start], (rho - 1 + bafke * 2 ** (logR / gamma) * ((1 - rho) * 2 + rho * psi)) / rho, 0)
        if nAraw + nBraw < 0:                                   # negative values
            nAraw, nBraw = 0, 0
        elif nAraw < 0:
            nBraw += nAraw
            nAraw = 0
        elif nBraw < 0:
            nAraw += nBraw
            nBraw = 0
        limitround = 0.5                                        # odd copy numbers
        nA = np.where(bafke == 0.5,
                      np.where(nAraw + nBraw > np.round(nAraw) + np.round(nBraw) + limitround,
                               np.round(nAraw) + 1,
                               np.where(nAraw + nBraw < np.round(nAraw) + np.round(nBraw) - limitround, np.round(nAraw), np.round(nAraw))),
                      np.round(nAraw))
        nB = np.where(bafke == 0.5,
                      np.where(nAraw + nBraw > np.round(nAraw) + np.round(nBraw) + limitround,
                               np.round(nBraw),
                               np.where(nAraw + nBraw < np.round(nAraw) + np.round(nBraw) - limitround, np.round(nBraw) - 1, np.round(nBraw))),
                      np.round(nBraw))
        seg.append([start, end, int(nA), int(nB)])
    seg = np.array(seg)
    for _ in range(20):
        seg2 = seg.copy()
        new_seg = []
        skipnext = False
        for i in range(len(seg2)):
            if not skipnext:
                if i != len(seg2) - 1 and seg2[i, 2] == seg2[i + 1, 2] and seg2[i, 3] == seg2[i + 1, 3]:
                    segline = [seg2[i, 0], seg2[i + 1, 1], seg2[i, 2], seg2[i, 3]]
                    skipnext = True
                else:
                    segline = seg2[i]
                new_seg.append(segline)
            else:
                skipnext = False
        seg = np.array(new_seg)
    return seg


def run_ascat(tumor_logr_file, tumor_baf_file, germline_genotypes_file, tumor_logr_segmented_file, tumor_baf_segmented_file,
              tumor_purity_ploidy_output_file, tumor_cna_output_file, gamma=1.0, min_ploidy=1.5, max_ploidy=5.5, min_purity=0.1, max_purity=1.05,
              sample_name="SAMPLE", where=None, stats=None, seen=None):
    read_table(tumor_logr_file)                                 # read and not used, as in the reference: a missing file fails here
    tumor_baf_dict, gg_table = read_table(tumor_baf_file), read_table(germline_genotypes_file)
    germline_genotypes_values = np.array(list(gg_table.values()))
    het_indices = np.where(germline_genotypes_values == 'False')[0]
    if len(het_indices) == 0:
        return
    logr_segmented, baf_segmented = read_table(tumor_logr_segmented_file), read_table(tumor_baf_segmented_file)
    tumor_baf_ori = np.array(list(tumor_baf_dict.values()))
    b = np.array([float(v) for v in baf_segmented.values()])
    r_ori = np.array([float(v) for v in logr_segmented.values()])
    r = r_ori[het_indices]

    s = make_segments(r, b)
    d = create_distance_matrix(s, gamma, min_ploidy, max_ploidy, min_purity, max_purity, where or _default_where(), stats)
    optima, psi_values, rho_values = find_optima(d, s, gamma, min_ploidy, max_ploidy, seen)
    if not optima:
        print("Could not find an optimal purity and ploidy value for {}!".format(sample_name))
        return
    optlim = np.min([opt[0] for opt in optima])
    for opt in optima:
        if opt[0] == optlim:
            psi = psi_values[int(opt[1])]
            rho = rho_values[int(opt[2])]
            if rho > 1:
                rho = 1
            goodnessOfFit = opt[4]
            break

    seg = copy_number_segments(rho, psi, gamma, b, r_ori, het_indices, len(germline_genotypes_values))
    nMajor, nMinor = np.zeros(len(r_ori)), np.zeros(len(r_ori))
    for row in seg:
        start, end, nA, nB = row
        nMajor[int(start):int(end) + 1] = nA
        nMinor[int(start):int(end) + 1] = nB
    n1all, n2all = np.zeros(len(r_ori)), np.zeros(len(r_ori))
    homo_indices = np.where(germline_genotypes_values == 'True')[0]
    n1all[het_indices] = np.where(tumor_baf_ori[het_indices].astype(float) <= 0.5, nMajor[het_indices], nMinor[het_indices])
    n2all[het_indices] = np.where(tumor_baf_ori[het_indices].astype(float) > 0.5, nMajor[het_indices], nMinor[het_indices])
    n1all[homo_indices] = np.where(tumor_baf_ori[homo_indices].astype(float) <= 0.5, nMajor[homo_indices] + nMinor[homo_indices], 0)
    n2all[homo_indices] = np.where(tumor_baf_ori[homo_indices].astype(float) > 0.5, nMajor[homo_indices] + nMinor[homo_indices], 0)
    ploidy = np.mean(n1all + n2all)

    keys = list(tumor_baf_dict.keys())
    lines = []
    for idx, seg_line in enumerate(seg):
        start_key = keys[int(seg_line[0]) if idx == 0 else int(seg_line[0]) + 1]      # every start but the first is one row late, as in the reference
        end_key = keys[int(seg_line[1])]
        lines.append(sample_name + '\t' + '\t'.join([start_key[0], start_key[1], end_key[1], str(seg_line[2]), str(seg_line[3])]) + '\n')
    with open(tumor_purity_ploidy_output_file, 'w') as f:
        f.write('Sample\tPurity\tPloidy\tGoodnessOfFit\n')
        f.write(sample_name + '\t' + str(rho) + '\t' + str(ploidy) + '\t' + str(goodnessOfFit) + '\n')
    with open(tumor_cna_output_file, 'w') as f:
        f.write('Sample\tChromosome\tStartPosition\tEndPosition\tnMajor\tnMinor\n')
        f.writelines(lines)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="run_ascat", description="Run ASCAT")
    ap.add_argument('--tumor_logr_file', type=str, default=None, help="Path of tumor sample LogR")
    ap.add_argument('--tumor_baf_file', type=str, default=None, help="Path of tumor sample BAF")
    ap.add_argument('--germline_genotypes_file', type=str, default=None, help="Path of germline genotypes")
    ap.add_argument('--tumor_logr_segmented_file', type=str, default=None, help="Path of tumor sample PCFed LogR")
    ap.add_argument('--tumor_baf_segmented_file', type=str, default=None, help="Path of tumor sample PCFed BAF")
    ap.add_argument('--tumor_purity_ploidy_output_file', type=str, default=None, help="Output path of estimated tumor sample purity and ploidy")
    ap.add_argument('--tumor_cna_output_file', type=str, default=None, help="Output path of tumor sample CNA file")
    ap.add_argument('--gamma', type=float, default=1.0, help="Value of gamma parameter")
    ap.add_argument('--min_ploidy', type=float, default=1.5, help="Value of min ploidy")
    ap.add_argument('--max_ploidy', type=float, default=5.5, help="Value of max ploidy")
    ap.add_argument('--min_purity', type=float, default=0.1, help="Value of min purity")
    ap.add_argument('--max_purity', type=float, default=1.05, help="Value of max purity")
    ap.add_argument('--sample_name', type=str, default="SAMPLE", help="Tumor sample name")
    ap.add_argument("--where", choices=("device", "host"), default=None, help="ours: where the grid is computed; default: device when a GPU is present")
    a = ap.parse_args(argv)
    run_ascat(a.tumor_logr_file, a.tumor_baf_file, a.germline_genotypes_file, a.tumor_logr_segmented_file, a.tumor_baf_segmented_file,
              a.tumor_purity_ploidy_output_file, a.tumor_cna_output_file, a.gamma, a.min_ploidy, a.max_ploidy, a.min_purity, a.max_purity, a.sample_name,
              a.where)
    return 0


if __name__ == "__main__":
    main(sys.argv[1:])
