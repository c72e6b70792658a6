"""Step 7, the last, of the Verdict chain (src/verdict/tag_germline_variant.py of the reference, run by src/cna_germline_tagging.py:157-197):
the calls of a VCF, the purity and the copy-number segments of run_ascat -> the same VCF with the PASS calls that look germline set to
LowQual and Verdict_Germline / Verdict_Somatic / Verdict_SubclonalSomatic appended to INFO.

    python -m clairs_to_amd tag_germline_variant --input_vcf_fn F --output_fn F --tumor_purity_ploidy_output_file F
           --tumor_cna_output_file F [--where device|host]

The hot path is, per PASS call, a linear scan of the segment table and up to four exact binomial tests.  Here all calls go through one
cto_tag_germline call (csrc/taggermline.hip: the rules, the kernel, the host path): the first segment in file order that holds the call,
the expected allele fractions, the p-values.  What reads them stays here, in the reference's order of comparisons: the builtin max and
min (the second argument wins only when strictly larger or smaller, so a NaN there never wins - the reference's `from numpy import *` was
written against them), numpy's log10 for the log-odds, the decision tree of lines 123-185 over arrays.

As in the reference: a missing purity or segment file, or a purity above 0.6, prints a warning and writes nothing; the input may be plain
or gzip / BGZF; header rows are kept as they are; rows are keyed by (contig, position), a later duplicate replacing the earlier row where
that one stood; AF is the AF (else VAF) field of FORMAT and the depth the third field of column 10, whatever FORMAT says; a PASS row is
written with its blanks stripped, every other row byte for byte.  Where the reference dies, so do we, with a message that names the row:
a row too short to parse, a depth that is not an integer, and, for a call inside a segment, no AF field, a depth below 1 or an AF that
puts more successes than trials."""
import argparse
import ctypes as C
import gzip
import io
import os
import sys

import numpy as np

ALPHA = 0.01


def _default_where():
    import torch
    return "device" if torch.cuda.is_available() else "host"


# ------------------------------------------------------------------------------------------------ the C calls
def _where_code(where):
    if where not in ("device", "host"):
        raise ValueError("where must be 'device' or 'host'")
    return 0 if where == "device" else 1


def tag_calls(ctg, pos, depth, freq, seg_chr, seg_start, seg_end, seg_nmaj, seg_nmin, purity, where="device", stats=None):
    """(seg, af, pv) of cto_tag_germline: per call the segment's index or -1, and four fractions and four p-values (G1, S1, G2, S2).
    stats: a dict that receives the call's cto_tag_germline_stats."""
    from ._lib import TagGermlineStats, check, lib
    code = _where_code(where)
    ctg, seg_chr = [np.ascontiguousarray(v, dtype=np.int32) for v in (ctg, seg_chr)]
    pos, depth, seg_start, seg_end, seg_nmaj, seg_nmin = [np.ascontiguousarray(v, dtype=np.int64) for v in (pos, depth, seg_start, seg_end, seg_nmaj, seg_nmin)]
    freq = np.ascontiguousarray(freq, dtype=np.float64)
    if not (ctg.shape == pos.shape == depth.shape == freq.shape and ctg.ndim == 1):
        raise ValueError("ctg, pos, depth and freq must be flat and of one length")
    if not (seg_chr.shape == seg_start.shape == seg_end.shape == seg_nmaj.shape == seg_nmin.shape and seg_chr.ndim == 1):
        raise ValueError("the five columns of the segment table must be flat and of one length")
    n = len(ctg)
    seg, af, pv = np.full(n, -1, dtype=np.int32), np.full((n, 4), np.nan), np.full((n, 4), np.nan)
    st = TagGermlineStats()
    check(lib.cto_tag_germline(ctg.ctypes.data, pos.ctypes.data, depth.ctypes.data, freq.ctypes.data, n, seg_chr.ctypes.data, seg_start.ctypes.data,
                               seg_end.ctypes.data, seg_nmaj.ctypes.data, seg_nmin.ctypes.data, len(seg_chr), float(purity), code, seg.ctypes.data,
                               af.ctypes.data, pv.ctypes.data, C.byref(st)))
    if stats is not None:
        for name, _ in TagGermlineStats._fields_:
            stats[name] = getattr(st, name)
    return seg, af, pv


def binom_two_sided(k, n, p, where="host"):
    """the two-sided p-values of cto_binom_two_sided: k successes in n trials against p"""
    from ._lib import check, lib
    code = _where_code(where)
    k, n = np.ascontiguousarray(k, dtype=np.int64), np.ascontiguousarray(n, dtype=np.int64)
    p = np.ascontiguousarray(p, dtype=np.float64)
    if not (k.shape == n.shape == p.shape and k.ndim == 1):
        raise ValueError("k, n and p must be flat and of one length")
    out = np.zeros(len(k))
    check(lib.cto_binom_two_sided(k.ctypes.data, n.ctypes.data, p.ctypes.data, len(k), code, out.ctypes.data))
    return out


# ------------------------------------------------------------------------------------------------ the files
class Row(object):
    __slots__ = ("row_str", "filter", "af")

    def __init__(self, row_str, filter, af):
        self.row_str, self.filter, self.af = row_str, filter, af


def read_vcf(vcf_fn):
    """(header, {(contig, position): Row}) as VcfReader(show_ref, keep_row_str, keep_af, skip_genotype, save_header) leaves them"""
    header, rows = "", {}
    if vcf_fn is None or not os.path.exists(vcf_fn):
        return header, rows
    with open(vcf_fn, "rb") as f:
        raw = f.read()
    if raw[:2] == b"\x1f\x8b":
        raw = gzip.decompress(raw)
    header_last_column = []
    for no, row in enumerate(io.TextIOWrapper(io.BytesIO(raw), newline=None)):
        try:
            columns = row.strip().split()
            if columns[0][0] == "#":
                header += row
                header_last_column = columns
                continue
            tumor_in_last = bool(len(header_last_column)) and header_last_column[-1].rstrip().lower() == "tumor"
            chromosome, position = columns[0], columns[1]
            FILTER = columns[6] if len(columns) >= 7 else None
            columns[2][0]                                       # the reference looks at it
            alternate, last_column = columns[4], columns[-1]
            last_column = last_column if not tumor_in_last else columns[-2]
            genotype = last_column.split(":")[0].replace("/", "|").replace(".", "0").split("|")
            try:
                genotype_1, genotype_2 = genotype
                total = int(genotype_1) + int(genotype_2)
                if '*' in alternate and (total != 3 or len(alternate.split(',')) != 2):
                    print('error with variant representation')
                    continue
            except ValueError:                                  # a genotype that is no pair of integers is read as unknown
                pass
            tag_list = columns[8].split(':')
            if 'AF' in tag_list or 'VAF' in tag_list:
                taf = float(columns[9].split(':')[tag_list.index('AF') if 'AF' in tag_list else tag_list.index('VAF')])
            else:
                taf = None
            rows[(chromosome, int(position))] = Row(row, FILTER, taf)
        except (IndexError, ValueError) as e:
            sys.exit("tag_germline_variant: cannot read line %d of %s (%s; the reference fails there): %r" % (no + 1, vcf_fn, e, row))
    return header, rows


def read_segments(segment_path):
    """the five columns of the copy-number table, by position, the header row left out; quotes stripped from the contig only"""
    seg_chr, seg_start, seg_end, cn_major, cn_minor = [], [], [], [], []
    with open(segment_path, 'r') as f:
        for idx, cna in enumerate(f.readlines()):
            if idx == 0:
                continue
            try:
                cna_columns = cna.strip().split('\t')
                fields = (str(cna_columns[1].strip('"')), int(cna_columns[2]), int(cna_columns[3]), int(cna_columns[4]), int(cna_columns[5]))
            except (IndexError, ValueError) as e:
                sys.exit("tag_germline_variant: cannot read line %d of %s (%s; the reference fails there): %r" % (idx + 1, segment_path, e, cna))
            for column, value in zip((seg_chr, seg_start, seg_end, cn_major, cn_minor), fields):
                column.append(value)
    return seg_chr, seg_start, seg_end, cn_major, cn_minor


# ------------------------------------------------------------------------------------------------ lines 113-185, over arrays
NONE, SUBCLONAL, GERMLINE, SOMATIC = 0, 1, 2, 3


def decide(frequency, p, af, pv):
    """what the decision tree does to every call with a segment: NONE, SUBCLONAL, GERMLINE or SOMATIC.  frequency: the calls' AF; p: the
    purity; af, pv: the n x 4 arrays of tag_calls (G1, S1, G2, S2)"""
    AF_G1, AF_S1, AF_G2, AF_S2 = af.T
    P_G1, P_S1, P_G2, P_S2 = pv.T
    with np.errstate(invalid="ignore", divide="ignore"):
        max_prob_germline = np.where(P_G2 > P_G1, P_G2, P_G1)               # max(P_G1, P_G2) of the builtins
        max_prob_somatic = np.where(P_S2 > P_S1, P_S2, P_S1)
        logodds = np.where(max_prob_somatic == 0, np.inf,
                           np.where(max_prob_germline == 0, -np.inf, np.log10(max_prob_germline) - np.log10(max_prob_somatic)))
        min_soma_EAF = np.where(AF_S2 < AF_S1, AF_S2, AF_S1)                # min(AF_S1, AF_S2) of the builtins
        min_germ_EAF = np.where(AF_G2 < AF_G1, AF_G2, AF_G1)
        pick = np.where
        neither = pick((p >= 0.3) & (frequency < 0.25) & (frequency < min_soma_EAF / 1.5) & (min_soma_EAF <= min_germ_EAF), SUBCLONAL,
                       pick((p >= 0.3) & (frequency < 0.25) & (frequency < min_germ_EAF / 2.0) & (min_germ_EAF < min_soma_EAF), SUBCLONAL,
                            pick((logodds < -5) & (max_prob_somatic > 1e-10), SOMATIC,
                                 pick((logodds > 5) & (max_prob_germline > 1e-4), GERMLINE, NONE))))
        return pick((frequency < 0.05) & (0.2 < p < 0.6), SUBCLONAL,
                    pick(frequency > 0.95, GERMLINE,
                         pick((max_prob_germline > ALPHA) & (max_prob_somatic < ALPHA), pick(logodds < 2, NONE, pick(frequency > 0.25, GERMLINE, NONE)),
                              pick((max_prob_germline < ALPHA) & (max_prob_somatic > ALPHA), pick(logodds > -2, NONE, SOMATIC),
                                   pick((max_prob_germline > ALPHA) & (max_prob_somatic > ALPHA), NONE,
                                        pick((max_prob_germline < ALPHA) & (max_prob_somatic < ALPHA), neither, NONE))))))


def tag_germline_variant(input_vcf_fn, output_fn, tumor_purity_ploidy_output_file, tumor_cna_output_file, where=None, stats=None):
    from .postprocess_vcf import compress_index_vcf
    tumor_purity_path, segment_path = tumor_purity_ploidy_output_file, tumor_cna_output_file
    if not os.path.exists(tumor_purity_path) or not os.path.exists(segment_path):
        print("[WARNING] Verdict can not obtain final results, not applying verdict tagging!")
        return
    tumor_purity = float(open(tumor_purity_path).read().rstrip().split('\n')[1].split('\t')[1])
    if tumor_purity > 0.6:
        print("[WARNING] Tumor purity estimation {} is higher than 0.6, not applying verdict tagging!".format(tumor_purity))
        return
    header, rows = read_vcf(input_vcf_fn)
    seg_chr, seg_start, seg_end, cn_major, cn_minor = read_segments(segment_path)

    ids = {}
    passed, split, ctg, pos, depth, freq, fatal = [], [], [], [], [], [], []
    for v in rows.values():
        if v.filter != 'PASS':
            continue
        columns = v.row_str.strip().split('\t')
        try:
            n = int(columns[9].strip().split(':')[2])
            at = int(columns[1])
        except (IndexError, ValueError) as e:
            sys.exit("tag_germline_variant: no integer depth or position (%s; the reference fails there) in the row %r" % (e, v.row_str))
        # what the reference would die of once a segment holds the call; such a call is sent with values that can be tested
        why = None
        if v.af is None:
            why = "no AF or VAF field"
        elif not np.isfinite(v.af):
            why = "cannot convert float %r to integer" % v.af
        elif n < 1:
            why = "n must be an integer not less than 1, but it is %d" % n
        else:
            k = round(n * v.af)
            if k < 0:
                why = "k must be an integer not less than 0, but it is %d" % k
            elif k > n:
                why = "k (%d) must not be greater than n (%d)." % (k, n)
        passed.append(v)
        split.append(columns)
        ctg.append(ids.setdefault(columns[0], len(ids)))
        pos.append(at)
        depth.append(1 if why else n)
        freq.append(0.0 if why else v.af)
        fatal.append(why)

    if passed:
        for values, what in ((pos, "position"), (seg_start, "segment start"), (seg_end, "segment end"), (cn_major, "nMajor"), (cn_minor, "nMinor"), (depth, "depth")):
            if values and not (-2 ** 62 < min(values) and max(values) < 2 ** 62):
                sys.exit("tag_germline_variant: a %s does not fit 63 bits" % what)
        seg, af, pv = tag_calls(ctg, pos, depth, freq, [ids.setdefault(c, len(ids)) for c in seg_chr], seg_start, seg_end, cn_major, cn_minor,
                                tumor_purity, where or _default_where(), stats)
        for i in np.flatnonzero(seg >= 0):
            if fatal[i]:
                sys.exit("tag_germline_variant: %s (the reference fails there) in the row %r" % (fatal[i], passed[i].row_str))
        inside = np.flatnonzero(seg >= 0)
        verdict = decide(np.array(freq, dtype=np.float64)[inside], tumor_purity, af[inside], pv[inside])
        for i, what in zip(inside, verdict):
            columns = split[i]
            if what == SUBCLONAL:
                columns[7] += ';Verdict_SubclonalSomatic'
            elif what == GERMLINE:
                columns[6] = 'LowQual'
                columns[7] += ';Verdict_Germline'
            elif what == SOMATIC:
                columns[7] += ';Verdict_Somatic'
        for v, columns in zip(passed, split):
            v.row_str = '\t'.join(columns) + '\n'

    with open(output_fn, 'w') as f:
        f.write(header)
        for v in rows.values():
            f.write(v.row_str)
    if os.path.exists(output_fn):
        compress_index_vcf(output_fn)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="tag_germline_variant", description="")
    ap.add_argument('--tumor_purity_ploidy_output_file', type=str, default=None, help="Path of the estimated tumor purity and ploidy")
    ap.add_argument('--tumor_cna_output_file', type=str, default=None, help="Path of the tumor copy-number segments")
    ap.add_argument('--input_vcf_fn', type=str, default=None, help="Input VCF")
    ap.add_argument('--output_fn', type=str, default=None, help="Output file path")
    ap.add_argument("--where", choices=("device", "host"), default=None, help="ours: where the tests are computed; default: device when a GPU is present")
    a = ap.parse_args(argv)
    tag_germline_variant(a.input_vcf_fn, a.output_fn, a.tumor_purity_ploidy_output_file, a.tumor_cna_output_file, a.where)
    return 0


if __name__ == "__main__":
    main(sys.argv[1:])
