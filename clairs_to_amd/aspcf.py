"""Step 5 of the Verdict chain (src/verdict/aspcf.py of the reference, run by src/cna_germline_tagging.py:130-140): the logR, BAF and
germline genotype tables -> the segmented logR of every probe and the segmented BAF of every heterozygous probe.

    python -m clairs_to_amd aspcf --tumor_logr_file F --tumor_baf_file F --germline_genotypes_file F --tumor_logr_pcfed_output_file F
           --tumor_baf_pcfed_output_file F [--penalty 1000] [--sample_name S] [--where device|host]

The hot path is the penalised least-squares recurrence that the reference's fastAspcf runs on every window of at most 1000 heterozygous
probes: here all windows of all chromosomes go through one cto_aspcf_windows call per penalty (csrc/aspcf.hip: the rules, the kernel, the
host path).  The running medians (cto_running_median) and the single-track recurrence of the homozygous stretches (cto_exact_pcf) are C
calls on the host.  Everything else that decides a printed byte - the tables' dict semantics, the runs of chromosome names, the
stretches, the winsorising, the window schedule and the merge of the windows' breakpoints, every mean - is numpy on the host, in the
reference's own operation order (np.mean / np.nanmean over the same slices; numpy scalars squared with ** 2, which is libm's pow).
What depends on the tables alone and not on the penalty is computed once, not once per penalty.  scipy is not imported.

As in the reference: the three tables are matched by row order, not by key; when no probe is heterozygous nothing is written; the
penalties tried are the given one, then 70, 100, 140 above it, until fewer than 800 distinct levels are left.

Deviations: a logR or BAF that is not a finite number is refused with a message naming the row (scipy's median filter orders NaN by no
stated rule, so no output could be pinned; get_logr_and_baf never writes one: its logR is the log2 of a positive ratio, its BAF a
count over a positive total).  Where the reference dies, so do we, with a message: no homozygous probe at all (it takes min() of an
empty list), and a homozygous stretch whose flanked span holds fewer than 12 values (it indexes an array with 'yhat')."""
import argparse
import ctypes as C
import math
import sys

import numpy as np

from .predict_germline_genotypes import read_table

MAX_WINDOW = 1000            # CTO_ASPCF_MAX_WINDOW of include/clairsto_amd.h; also the reference's window size w
WINDOW_OVERLAP = 100         # d of fastAspcf
KMIN = 6
MEDIAN_K = 25
TAU = 2.5


def _default_where():
    import torch
    return "device" if torch.cuda.is_available() else "host"


# ------------------------------------------------------------------------------------------------ the C calls
def running_median(x, k):
    """medianFilter: the running median of width 2 k + 1 (cut to the array when longer), ends reflected"""
    from ._lib import check, lib
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty(len(x), dtype=np.float64)
    check(lib.cto_running_median(x.ctypes.data, len(x), int(k), out.ctypes.data))
    return out


def exact_pcf(y, kmin, gamma):
    """exactPcf: every value's segment average; the mean of all below 2 * kmin values"""
    from ._lib import check, lib
    y = np.ascontiguousarray(y, dtype=np.float64)
    yhat = np.zeros(len(y))
    if len(y) < 2 * kmin:
        yhat[:] = np.mean(y)
        return yhat
    check(lib.cto_exact_pcf(y.ctypes.data, len(y), int(kmin), float(gamma), yhat.ctypes.data))
    return yhat


def aspcf_windows(y1, y2, win_lo, win_hi, v1, v2, kmin, gamma, where="device", stats=None, want_cost=False):
    """best_split (and best_cost with want_cost) of cto_aspcf_windows, concatenated per window.  where: "device" or "host".  stats: a
    dict that receives the call's cto_aspcf_stats."""
    from ._lib import AspcfStats, check, lib
    if where not in ("device", "host"):
        raise ValueError("where must be 'device' or 'host'")
    y1 = np.ascontiguousarray(y1, dtype=np.float64)
    y2 = np.ascontiguousarray(y2, dtype=np.float64)
    win_lo = np.ascontiguousarray(win_lo, dtype=np.int64)
    win_hi = np.ascontiguousarray(win_hi, dtype=np.int64)
    v1 = np.ascontiguousarray(v1, dtype=np.float64)
    v2 = np.ascontiguousarray(v2, dtype=np.float64)
    if y1.ndim != 1 or y1.shape != y2.shape or win_lo.ndim != 1 or not (win_lo.shape == win_hi.shape == v1.shape == v2.shape):
        raise ValueError("y1, y2 and the four per-window arrays must be flat and of matching lengths")
    total = max(0, int(np.sum(win_hi - win_lo)))                # a negative length is the C call's to refuse
    split = np.zeros(total, dtype=np.int32)
    cost = np.zeros(total, dtype=np.float64) if want_cost else None
    st = AspcfStats()
    check(lib.cto_aspcf_windows(y1.ctypes.data, y2.ctypes.data, len(y1), win_lo.ctypes.data, win_hi.ctypes.data, len(win_lo), v1.ctypes.data,
                                v2.ctypes.data, int(kmin), float(gamma), 0 if where == "device" else 1, split.ctypes.data,
                                cost.ctypes.data if want_cost else None, C.byref(st)))
    if stats is not None:
        for name, _ in AspcfStats._fields_:
            stats[name] = getattr(st, name)
    return (split, cost) if want_cost else split


# ------------------------------------------------------------------------------------------------ small numpy pieces
def mad_of_residuals(d):
    return np.median(np.abs(d - np.median(d)))


def mad_wins(x, tau, k):
    """madWins: x pulled to within tau MADs of its running median"""
    if len(x) == 0:
        return np.zeros(0)
    xhat = running_median(x, k)
    d = x - xhat
    z = tau * mad_of_residuals(d)
    clipped = np.copy(d)
    clipped[d < -z] = -z
    clipped[d > z] = z
    return xhat + clipped


def get_mad(x, k=MEDIAN_K):
    """getMad: the MAD of the non-zero values around their running median; NaN when there is none"""
    x = x[x != 0]
    if len(x) == 0:
        return np.float64(np.nan)
    return mad_of_residuals(x - running_median(x, k))


def run_lengths(a):
    n = len(a)
    if n == 0:
        return np.array([], dtype=int)
    ends = np.append(np.where(np.array(a[1:] != a[:-1]))[0], n - 1)
    return np.diff(np.append(-1, ends))


def levels_of_runs(shape, values):
    """one np.nanmean of `values` per run of equal neighbours in `shape`, spread over the run"""
    out, lo = [], 0
    for length in run_lengths(shape):
        out.append(np.full(length, np.nanmean(values[lo:lo + length])))
        lo += length
    return np.concatenate(out) if out else np.array([], dtype=float)


def fill_zeros_and_nans(x):
    """fillNA(zeroIsNA=True): zeros and NaN replaced by linear interpolation between their neighbours"""
    x = x.copy()
    x[x == 0] = np.nan
    known = np.where(~np.isnan(x))[0]
    x[np.isnan(x)] = np.interp(np.where(np.isnan(x))[0], known, x[known])
    return x


def chromosome_runs(keys):
    """row indices per stretch of equal chromosome names in table order; a name that comes back starts a new run"""
    runs, current = [], None
    for i, (ctg, _) in enumerate(keys):
        if ctg != current:
            runs.append([])
            current = ctg
        runs[-1].append(i)
    return runs


def homozygous_stretches(runs, gg):
    """predictGermlineHomozygousStretches: [run, first row, last row] of every stretch of homozygous probes at least homthres long"""
    share = np.sum(gg == "True") / len(gg)
    if share == 0.0:
        raise ValueError("aspcf: no probe is homozygous (the reference fails there, on min() of an empty list)")
    threshold = 1 if share == 1.0 else math.ceil(math.log(0.001, share))
    out = []
    for r, rows in enumerate(runs):
        stretch = []
        for row in rows:
            if gg[row] == "True":
                stretch.append(row)
                continue
            if len(stretch) >= threshold:
                out.append([r, stretch[0], stretch[-1]])           # threshold >= 1: never empty
            stretch = []
        if stretch and len(stretch) >= threshold:
            out.append([r, stretch[0], stretch[-1]])
    return out or [[0, 0, 0]]


# ------------------------------------------------------------------------------------------------ what does not depend on the penalty
class Window:
    __slots__ = ("a", "b", "lo", "hi", "sd1", "sd2", "fit")


def window_schedule(n):
    """(startw, stopw) of fastAspcf: w = 1000, d = 100, the first window ends at 900, the last one is pulled back to end at n + 100"""
    w, d = MAX_WINDOW, WINDOW_OVERLAP
    a, b = -d, w - d
    out = []
    while True:
        out.append((a, b))
        if b >= n + d:
            return out
        a = min(b - 2 * d + 1, n - 2 * d)
        b = a + w


class Chromosome:
    """one run of rows: its logR, the heterozygous probes' averaged logR and winsorised BAF, and the windows of fastAspcf with their MADs"""

    def __init__(self, rows, logr, baf, gg):
        self.rows = rows
        self.lr = lr = logr[rows]
        lrwins = mad_wins(lr, TAU, MEDIAN_K)
        het = gg[rows] == "False"
        bafsel = baf[rows][het]
        self.mirrored = mirrored = mad_wins(np.where(bafsel > 0.5, bafsel, 1 - bafsel), TAU, MEDIAN_K)
        self.baf = np.where(bafsel > 0.5, mirrored, 1 - mirrored)
        self.het = h = np.where(het)[0]
        self.y1 = self.y2 = None
        self.windows = []
        if len(h) == 0:
            return
        if len(h) == 1:
            first, last = [0], [len(lr) - 1]
        else:
            mid = np.concatenate(([0], (h[:-1] + h[1:]) / 2, [len(lr)]))
            first, last = np.ceil(mid[:-1]).astype(int), np.floor(mid[1:]).astype(int)
        self.y1 = np.full(len(h), np.nan)
        for i in range(len(h)):
            self.y1[i] = np.nanmean(lrwins[first[i]:last[i] + 1])
        if len(h) < KMIN:
            return
        self.y2 = np.where(self.baf > 0.5, 1 - self.baf, self.baf)              # the flip of every window, taken once
        n = len(h)
        for a, b in window_schedule(n):
            w = Window()
            w.a, w.b, w.lo, w.hi = a, b, max(0, a), min(b, n)
            w.sd1, w.sd2 = get_mad(self.y1[w.lo:w.hi]), get_mad(self.y2[w.lo:w.hi])
            w.fit = bool(not np.isnan(w.sd1) and not np.isnan(w.sd2) and w.sd1 != 0 and w.sd2 != 0)
            self.windows.append(w)


# ------------------------------------------------------------------------------------------------ one penalty
def window_breakpoints(chroms, gamma, where, stats):
    """{(chromosome, window): breakpoints as aspcfpart returns them} for every window that passes the MAD test: one C call"""
    y1, y2, lo, hi, v1, v2, who, off = [], [], [], [], [], [], [], 0
    out = {}
    for c, ch in enumerate(chroms):
        if ch.y2 is None:
            continue
        for k, w in enumerate(ch.windows):
            if not w.fit:
                continue
            if w.hi - w.lo < 2 * KMIN:
                out[(c, k)] = [0]
                continue
            who.append((c, k))
            lo.append(off + w.lo)
            hi.append(off + w.hi)
            v1.append(w.sd1 ** 2)
            v2.append(w.sd2 ** 2)
        y1.append(ch.y1)
        y2.append(ch.y2)
        off += len(ch.y1)
    if not who:
        return out
    st = {}
    split = aspcf_windows(np.concatenate(y1), np.concatenate(y2), lo, hi, v1, v2, KMIN, gamma, where, st)
    if stats is not None:
        for key, v in st.items():
            stats[key] = v if key == "host_path" else stats.get(key, 0) + v
    at = 0
    for (c, k), a, b in zip(who, lo, hi):
        n = b - a
        s = split[at:at + n]
        at += n
        w, ch = chroms[c].windows[k], chroms[c]
        bp = [n]
        while n > 0:
            n = int(s[n - 1])
            bp.append(n)
        bp = np.array(bp) + w.lo - 1
        use_from, use_to = max(0, w.a + WINDOW_OVERLAP), min(len(ch.y1), w.b - WINDOW_OVERLAP)
        out[(c, k)] = bp[(bp >= use_from) & (bp <= use_to)].tolist()
    return out


def fit_levels(c, ch, parts):
    """fastAspcf after its windows: the merged breakpoints, then per segment the mean logR and the BAF level (0.5 unless 2 sd away)"""
    n = len(ch.y1)
    breakpts, var2, nseg = [0], 0, 0
    for k, w in enumerate(ch.windows):
        if not w.fit:
            continue
        part = np.array(parts[(c, k)])
        breakpts.extend(part[part > breakpts[-1]])              # in the part's own (descending) order, as the reference does
        var2 += w.sd2 ** 2
        nseg += 1
    breakpts = list(np.unique(breakpts + [n]))
    sd2 = np.sqrt(var2 / max(nseg, 1))
    yhat1, yhat2 = np.full(n, np.nan), np.full(n, np.nan)
    for lo, hi in zip(breakpts[:-1], breakpts[1:]):
        yhat1[lo:hi] = np.mean(ch.y1[lo:hi])
        side = ch.baf[lo:hi]
        mu = np.mean(np.abs(side - 0.5)) if len(side) else 0
        if np.sqrt(sd2 ** 2 + mu ** 2) < 2 * sd2:
            mu = 0
        yhat2[lo:hi] = mu + 0.5
    return yhat1, yhat2


def spread_over_probes(ch, level):
    """the heterozygous probes' levels over all probes of the chromosome, each change of level placed where the raw logR fits best"""
    lr, h = ch.lr, ch.het
    pieces, n_done = [], 0
    for p in range(len(level)):
        if p == 0:
            new = [np.full(h[p], level[p])]
        elif p == len(level) - 1:
            new = [np.full(len(lr) - h[p], level[p])]
        else:
            lo, hi = h[p], h[p + 1]
            if level[p] == level[p + 1]:
                new = [np.full(hi - lo, level[p])]
            else:
                d = np.array([])
                for bp in range(hi - lo):
                    dis = np.sum(np.abs(lr[lo:lo + bp] - level[p]))
                    dis += np.sum(np.abs(lr[lo + bp + 1:hi] - level[p + 1]))
                    d = np.append(d, dis)
                cut = np.argmin(d)
                new = [np.full(cut, level[p]), np.full(hi - lo - cut, level[p + 1])]
        pieces += new
        n_done += sum(len(x) for x in new)
    pieces.append(np.full(len(lr) - n_done, level[-1]))         # a negative count raises, as in the reference
    return np.concatenate(pieces)


def replace_by_stretches(seg, logr, ch, stretches, gamma):
    """a homozygous stretch whose own fit (exactPcf of its winsorised logR, 100 probes of flank) lies more than 0.3 from the levels at
    more than five probes takes its own fit there"""
    first, last = np.min(ch.rows), np.max(ch.rows)
    for _, s, e in stretches:
        lo2, hi2 = max(s - 100, first), min(e + 100, last)
        lo3, hi3 = max(s - 5, first), min(e + 5, last)
        span = logr[lo2:hi2 + 1]
        ok = ~np.isnan(span)
        wins = mad_wins(span[ok], TAU, MEDIAN_K)
        if len(wins) < 2 * KMIN:
            raise IndexError("aspcf: the homozygous stretch of rows %d-%d spans %d values, fewer than %d (the reference fails there)"
                             % (s, e, len(wins), 2 * KMIN))
        own = np.full(len(span), np.nan)
        own[ok] = exact_pcf(wins, KMIN, int(gamma / 4))
        own = own[lo3 - lo2:hi3 - lo2 + 1]
        cur = seg[lo3:hi3 + 1]
        if len(own) != len(cur):
            own = own[:len(cur)]
        dif = np.abs(own - cur)
        if not np.any(np.isnan(dif)) and np.sum(dif > 0.3) > 5:
            seg[lo3:hi3 + 1] = np.where(dif > 0.3, own, cur)
    return seg


def segment_once(chroms, logr, stretches, gamma, where, stats):
    parts = window_breakpoints(chroms, gamma, where, stats)
    seg, baf_seg = np.array([]), np.array([])
    for c, ch in enumerate(chroms):
        if ch.y1 is not None:
            if len(ch.y1) < KMIN:
                level, baf_level = np.full(len(ch.y1), np.mean(ch.y1)), np.full(len(ch.y1), np.mean(ch.mirrored))
            else:
                level, baf_level = fit_levels(c, ch, parts)
            seg = np.concatenate((seg, levels_of_runs(spread_over_probes(ch, level), ch.lr)))
            baf_seg = np.concatenate((baf_seg, baf_level))
        else:
            seg = np.concatenate((seg, np.full(len(ch.lr), np.nanmean(ch.lr))))
        seg = replace_by_stretches(seg, logr, ch, [s for s in stretches if s[0] == c], gamma)
    seg = fill_zeros_and_nans(seg)
    out, lo, prev = [], 0, 0
    for length in run_lengths(seg):
        level = np.nanmean(logr[lo:lo + length])
        if np.isnan(level):
            level = prev
        else:
            prev = level
        out.append(np.full(length, level))
        lo += length
    return np.concatenate(out), baf_seg


def finite_column(table, what):
    v = np.array(list(table.values())).astype(float)
    bad = np.where(~np.isfinite(v))[0]
    if len(bad):
        key = list(table)[bad[0]]
        sys.exit("aspcf: the %s of %s:%s is '%s', not a finite number" % (what, key[0], key[1], table[key]))
    return v


def aspcf(tumor_logr_file, tumor_baf_file, germline_genotypes_file, logr_output_file, baf_output_file, penalty=1000, sample_name="SAMPLE",
          where=None, stats=None):
    logr_table, baf_table, gg_table = read_table(tumor_logr_file), read_table(tumor_baf_file), read_table(germline_genotypes_file)
    gg = np.array(list(gg_table.values()))
    het_rows = np.where(gg == "False")[0]
    if len(het_rows) == 0:
        return
    logr, baf = finite_column(logr_table, "logR"), finite_column(baf_table, "BAF")
    runs = chromosome_runs(baf_table)
    stretches = homozygous_stretches(runs, gg)
    chroms = [Chromosome(rows, logr, baf, gg) for rows in runs]
    where = where or _default_where()
    for gamma in [g for g in sorted({penalty, 70, 100, 140}) if g >= penalty]:
        seg, baf_seg = segment_once(chroms, logr, stretches, gamma, where, stats)
        if len(np.unique(seg)) < 800:
            break
    baf_out = 1 - baf_seg
    baf_keys = list(baf_table)
    header = "Chromosome\tPosition\t%s\n" % sample_name
    logr_lines = ["%s\t%s\t%s\n" % (ctg, pos, str(seg[i])) for i, (ctg, pos) in enumerate(logr_table)]
    baf_lines = {baf_keys[row]: str(baf_out[i]) for i, row in enumerate(het_rows)}
    with open(logr_output_file, "w") as f:
        f.write(header)
        f.writelines(logr_lines)
    with open(baf_output_file, "w") as f:
        f.write(header)
        f.writelines("%s\t%s\t%s\n" % (ctg, pos, v) for (ctg, pos), v in baf_lines.items())


def main(argv=None):
    ap = argparse.ArgumentParser(prog="aspcf", description="Run ASPCF")
    ap.add_argument("--tumor_logr_file", type=str, default=None)
    ap.add_argument("--tumor_baf_file", type=str, default=None)
    ap.add_argument("--germline_genotypes_file", type=str, default=None)
    ap.add_argument("--tumor_logr_pcfed_output_file", type=str, default=None)
    ap.add_argument("--tumor_baf_pcfed_output_file", type=str, default=None)
    ap.add_argument("--penalty", type=int, default=1000)
    ap.add_argument("--sample_name", type=str, default="SAMPLE")
    ap.add_argument("--where", choices=("device", "host"), default=None, help="ours: where the window fits run; default: device when a GPU is present")
    a = ap.parse_args(argv)
    aspcf(a.tumor_logr_file, a.tumor_baf_file, a.germline_genotypes_file, a.tumor_logr_pcfed_output_file, a.tumor_baf_pcfed_output_file, a.penalty,
          a.sample_name, a.where)
    return 0


if __name__ == "__main__":
    main(sys.argv[1:])
