"""The reference's src/compare_vcf.py: a run's calls against a truth set -> the table of precision, recall and F1 its quick demos end with.
The files are parsed here as the reference parses them; the four loops over the two dicts, the BED lookups and the cut-off sweeps of
--output_best_f1_score and --roc_fn are one cto_compare_calls call (csrc/comparevcf.hip: the twelve rules, the kernels, the host path);
--min_af without --low_af_path is cal_af_distribution.cal_af, one pass over the BAM instead of one samtools process per truth variant.

    python -m clairs_to_amd compare_vcf --truth_vcf_fn TRUTH --input_vcf_fn CALLS [--bed_fn BED] [--ctg_name CTG --ctg_start S --ctg_end E]
        [--input_filter_tag PASS] [--output_dir DIR] [--output_fn TABLE] [--benchmark_indel] [--output_best_f1_score] [--roc_fn ROC]
        [--strat_bed_fn BED[,BED..]] [--min_af AF --tumor_bam_fn BAM | --low_af_path ROWS] [--where device|host]

The device supplies integers only: precision, recall and F1 are cal_metrics() on those counts, and the cut-off lists are built by the
reference's own expressions (`set([int(q) ...])`, `set(qual_list)`), so their order is CPython's set order on both sides.

Quirks kept (each pinned by tests/golden/compare_vcf.json.gz):
  * Position.genotype is a list: `genotype != (0, 0)` always holds and the two `== (0, 0)` skips never fire; --skip_genotyping False compares
    the lists;
  * `if tp_snv or is_snv_truth` tests the running count: once one SNV has matched, every later match joins tp_set, whatever its type;
  * --benchmark_indel deletes SNV and multi-allelic records from the input dict, but a key --high_confident_only marked leaves that loop
    before the deletion (and is skipped later);
  * --high_confident_only is a string: any value, "False" too, switches it on;
  * the FP BED passes everything when its tree has no contig at all; a stratification BED that names no matching contig fails every key;
  * the truth loop tests low_qual_truth before the stratification BEDs, the input loop after;
  * the best-F1 sweep counts len(fn_set), the ROC file fn_snv;
  * the low-AF key is int(pos) with --ctg_name and (ctg, int(pos)) without;
  * --output_path is read by cal_af: with it the rows go to that file and nothing comes back, and the reference fails on None.
Where the reference raises, the run ends with `compare_vcf: ...` naming the cause."""
import argparse
import ctypes as C
import gzip
import os
import sys
from collections import OrderedDict

import numpy as np

from ._cli import add_ignored, str2bool, str_none
from .cal_af_distribution import _default_where, cal_af, read_vcf

HIGHCONF, H, LOWAF = 1, 2, 4                                      # CTO_CMP_*: the flag byte of a record
FP, TP, FN, FP_FN, TRUTH, KEPT = 1, 2, 4, 8, 16, 32               # the set bits that come back
COUNTERS = ("tp_snv", "tp_ins", "tp_del", "fp_snv", "fp_ins", "fp_del", "fn_snv", "fn_ins", "fn_del", "gt_mismatch", "input_out_of_bed",
            "truth_out_of_bed", "input_out_of_strat_bed", "truth_out_of_strat_bed", "n_input_left", "n_truth_left")
MAX_SETS = 30

major_contigs_order = ["chr" + str(a) for a in list(range(1, 23)) + ["X", "Y"]] + [str(a) for a in list(range(1, 23)) + ["X", "Y"]]


def sort_key(item):
    order_map = {value: index for index, value in enumerate(major_contigs_order)}
    return order_map[item[0]], item[1]


def cal_metrics(tp, fp, fn):
    precision = tp / (tp + fp) if (tp + fp) > 0 else 0.0
    recall = tp / (tp + fn) if (tp + fn) > 0 else 0.0
    f1_score = 2 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0
    return round(precision, 4), round(recall, 4), round(f1_score, 4)


class BedTree(object):
    """what bed_tree_from() keeps of a BED file: per contig the sorted, merged 0-based [start, end) intervals.  len() is the number of
    contigs the file named, as len() of the reference's dict of interval trees."""

    def __init__(self):
        self.intervals = OrderedDict()                            # contig -> (starts, ends), int64, ascending, ends[k] <= starts[k + 1]

    def __len__(self):
        return len(self.intervals)


def bed_tree_from(bed_file_path, contig_name=None):
    """shared/interval_tree.py:8-77 as compare_vcf calls it: plain or gzip, `#` rows skipped, rows of other contigs skipped when contig_name is
    given, start == end widened by one.  is_region_in(tree, contig, pos - 1, pos) asks whether any interval overlaps, so merging the
    intervals changes no answer."""
    tree = BedTree()
    if bed_file_path is None or bed_file_path == "":
        return tree
    if not os.path.exists(bed_file_path):
        return tree                                               # `gzip -fdc` prints its complaint and the reference reads nothing
    with open(bed_file_path, "rb") as f:
        gz = f.read(2) == b"\x1f\x8b"
    rows = {}
    with (gzip.open(bed_file_path, "rt") if gz else open(bed_file_path)) as fo:
        for row_id, row in enumerate(fo):
            if row[0] == "#":
                continue
            columns = row.strip().split()
            ctg_name = columns[0]
            if contig_name is not None and ctg_name != contig_name:
                continue
            ctg_start, ctg_end = int(columns[1]), int(columns[2])
            if ctg_end < ctg_start or ctg_start < 0 or ctg_end < 0:
                sys.exit("[ERROR] Invalid bed input in {}-th row {} {} {}".format(row_id + 1, ctg_name, ctg_start, ctg_end))
            if ctg_end >= 2 ** 62:
                sys.exit("compare_vcf: BED row {} of {} is out of range".format(row_id + 1, bed_file_path))
            if ctg_start == ctg_end:
                ctg_end += 1
            rows.setdefault(ctg_name, []).append((ctg_start, ctg_end))
    for ctg, ivs in rows.items():
        ivs.sort()
        starts, ends = [], []
        for s, e in ivs:
            if ends and s <= ends[-1]:
                ends[-1] = max(ends[-1], e)
            else:
                starts.append(s)
                ends.append(e)
        tree.intervals[ctg] = (np.array(starts, dtype=np.int64), np.array(ends, dtype=np.int64))
    return tree


def pack_beds(trees, contigs):
    """the BED sets of cto_compare_calls: (named, off, start, end) over the contig ids of `contigs` (name -> id)"""
    n_ctg = len(contigs)
    named = np.array([len(t) for t in trees], dtype=np.int32)
    off = np.zeros(len(trees) * n_ctg + 1, dtype=np.int64)
    starts, ends = [], []
    by_id = sorted(contigs, key=contigs.get)
    for s, t in enumerate(trees):
        for c, name in enumerate(by_id):
            a, b = t.intervals.get(name, ((), ()))
            starts.append(np.asarray(a, dtype=np.int64))
            ends.append(np.asarray(b, dtype=np.int64))
            off[s * n_ctg + c + 1] = off[s * n_ctg + c] + len(a)
    cat = lambda parts: np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros(0, dtype=np.int64)
    return named, off, cat(starts), cat(ends)


def compare_calls(inp, tru, beds, n_ctg, benchmark_indel=False, high_confident_only=False, skip_genotyping=True, validate_phase=0, cutoffs=(),
                  roc_cutoffs=(), where="device", host_threads=0, stats=None):
    """cto_compare_calls on parallel arrays.  inp / tru: dicts of ctg, pos, ref_len, alt_len, n_alt, allele (int32 [n]), gt (int32 [n, 2]),
    flags (uint8 [n]) and, for inp, qual (float64 [n]); beds: (named, off, start, end) as pack_beds gives them.  Returns a dict: input_sets,
    truth_sets (uint8), counters (name -> int), sweep and roc_sweep (int64 [n, 2]: fp_set, tp_set records with QUAL >= the cut-off)."""
    from ._lib import CompareBeds, CompareRecords, CompareStats, check, lib
    if where not in ("device", "host"):
        raise ValueError("where must be 'device' or 'host'")
    keep = []

    def arr(x, dtype):
        a = np.ascontiguousarray(x, dtype=dtype)
        keep.append(a)
        return a

    def records(r, with_qual):
        n = len(r["pos"])
        cols = [arr(r[k], np.int32) for k in ("ctg", "pos", "ref_len", "alt_len", "n_alt", "allele")]
        gt = arr(r["gt"], np.int32).reshape(n, 2)
        qual = arr(r["qual"], np.float64) if with_qual else None
        flags = arr(r["flags"], np.uint8)
        if any(len(c) != n for c in cols) or len(flags) != n or (qual is not None and len(qual) != n):
            raise ValueError("the columns of a record table differ in length")
        ptr = [c.ctypes.data for c in cols] + [gt.ctypes.data, qual.ctypes.data if qual is not None else None, flags.ctypes.data]
        return CompareRecords(*ptr, n), cols, n

    rin, _, n_in = records(inp, True)
    rtr, tcols, n_tr = records(tru, False)
    keys = (tcols[0].astype(np.int64) << 32) | (tcols[1].astype(np.int64) & 0xFFFFFFFF)
    order = arr(np.argsort(keys, kind="stable"), np.int32)
    skeys = arr(keys[order], np.int64)
    named, off, start, end = (arr(beds[0], np.int32), arr(beds[1], np.int64), arr(beds[2], np.int64), arr(beds[3], np.int64))
    cb = CompareBeds(len(named), n_ctg, named.ctypes.data, off.ctypes.data, start.ctypes.data, end.ctypes.data)
    cut, roc = arr(cutoffs, np.float64), arr(roc_cutoffs, np.float64)
    in_sets, tr_sets = np.zeros(n_in, dtype=np.uint8), np.zeros(n_tr, dtype=np.uint8)
    counters = np.zeros(len(COUNTERS), dtype=np.int64)
    sweep, roc_sweep = np.zeros((len(cut), 2), dtype=np.int64), np.zeros((len(roc), 2), dtype=np.int64)
    st = CompareStats()
    stream = None
    if where == "device":
        from ._lib import current_stream_ptr
        stream = C.c_void_p(current_stream_ptr())
    check(lib.cto_compare_calls(C.byref(rin), C.byref(rtr), skeys.ctypes.data, order.ctypes.data, C.byref(cb), int(bool(benchmark_indel)),
                                int(bool(high_confident_only)), int(bool(skip_genotyping)), int(validate_phase), cut.ctypes.data, len(cut),
                                roc.ctypes.data, len(roc), 0 if where == "device" else 1, int(host_threads), stream, in_sets.ctypes.data,
                                tr_sets.ctypes.data, counters.ctypes.data, sweep.ctypes.data, roc_sweep.ctypes.data, C.byref(st)))
    if stats is not None:
        for name, _ in CompareStats._fields_:
            stats[name] = getattr(st, name)
    return dict(input_sets=in_sets, truth_sets=tr_sets, counters=dict(zip(COUNTERS, (int(c) for c in counters))), sweep=sweep, roc_sweep=roc_sweep)


def sweep_counts(values, sets, cutoffs, where="device", host_threads=0):
    """cto_compare_sweep: int64 [n_cutoffs, 2] - the values with FP, with TP in `sets` that are >= each cut-off"""
    from ._lib import check, lib
    v, s, c = np.ascontiguousarray(values, dtype=np.float64), np.ascontiguousarray(sets, dtype=np.uint8), np.ascontiguousarray(cutoffs, dtype=np.float64)
    if len(v) != len(s):
        raise ValueError("one set byte per value")
    out = np.zeros((len(c), 2), dtype=np.int64)
    stream = None
    if where == "device":
        from ._lib import current_stream_ptr
        stream = C.c_void_p(current_stream_ptr())
    check(lib.cto_compare_sweep(v.ctypes.data, s.ctypes.data, len(v), c.ctypes.data, len(c), 0 if where == "device" else 1, int(host_threads), stream,
                                out.ctypes.data))
    return out


def _as_float(qual):
    """the reference's `float(qual) if qual is not None else qual`, with its bare except: None where there is no number"""
    try:
        return float(qual) if qual is not None else None
    except Exception:
        return None


def _table(variant_dict, contigs, alleles, ctg_name, low_af_truth, with_h):
    """the parallel arrays of one dict, in dict order"""
    n = len(variant_dict)
    t = dict(ctg=np.zeros(n, np.int32), pos=np.zeros(n, np.int32), ref_len=np.zeros(n, np.int32), alt_len=np.zeros(n, np.int32), n_alt=np.zeros(n, np.int32),
             allele=np.zeros(n, np.int32), gt=np.zeros((n, 2), np.int32), qual=np.full(n, np.nan), flags=np.zeros(n, np.uint8))
    for i, (key, v) in enumerate(variant_dict.items()):
        pos = key if ctg_name is not None else key[1]
        if not -2 ** 31 <= pos < 2 ** 31:
            sys.exit("compare_vcf: position {} is out of range".format(pos))
        contig = ctg_name if ctg_name is not None else key[0]
        ref, alt = v.reference_bases, v.alternate_bases[0]
        t["ctg"][i] = contigs.setdefault(contig, len(contigs))
        t["pos"][i] = pos
        t["ref_len"][i], t["alt_len"][i], t["n_alt"][i] = len(ref), len(alt), len(v.alternate_bases)
        t["allele"][i] = alleles.setdefault((ref, alt), len(alleles))
        t["gt"][i] = v.genotype
        q = _as_float(v.qual)
        if q is not None:
            t["qual"][i] = q
        flags = HIGHCONF if "PASS;HighConf" in v.row_str else 0
        if with_h and "H" in v.row_str.rstrip().split("\t")[7].split(";"):
            flags |= H
        if key in low_af_truth:
            flags |= LOWAF
        t["flags"][i] = flags
    return t


def compare_vcf(args):
    """src/compare_vcf.py:82-538, in its order and with its printed lines"""
    ctg_name = args.ctg_name
    if ctg_name is not None and "," in ctg_name:
        sys.exit("compare_vcf: --ctg_name {}: the reference reads the keys of several contigs as positions and raises; give one contig or "
                 "none".format(ctg_name))
    benchmark_indel = args.benchmark_indel
    high_confident_only = bool(args.high_confident_only)          # a string in the reference: any value switches it on
    where = getattr(args, "where", None) or _default_where()

    fp_bed_tree = bed_tree_from(args.bed_fn, ctg_name)
    strat_bed_tree_list = []
    if args.strat_bed_fn is not None:
        strat_bed_tree_list = [bed_tree_from(fn, ctg_name) for fn in args.strat_bed_fn.split(",")]
    if 1 + len(strat_bed_tree_list) > MAX_SETS:
        sys.exit("compare_vcf: more than {} stratification BEDs".format(MAX_SETS - 1))
    for name, fn in (("truth", args.truth_vcf_fn), ("input", args.input_vcf_fn)):
        if fn is None:
            sys.exit("compare_vcf: --{}_vcf_fn is required".format(name))
        if not os.path.exists(fn):
            sys.exit("[ERROR] file %s not found" % fn)

    truth_variant_dict = read_vcf(args.truth_vcf_fn, ctg_name, args.truth_filter_tag, ctg_start=args.ctg_start, ctg_end=args.ctg_end,
                                  skip_genotype=args.skip_genotyping)
    input_variant_dict = read_vcf(args.input_vcf_fn, ctg_name, args.input_filter_tag, ctg_start=args.ctg_start, ctg_end=args.ctg_end,
                                  skip_genotype=args.skip_genotyping, keep_af=True, min_qual=args.min_qual, max_qual=args.max_qual,
                                  discard_indel=not benchmark_indel)

    low_af_truth = set()
    result_dict = None
    if args.min_af is not None:
        if args.low_af_path is None or not os.path.exists(args.low_af_path):
            if args.tumor_bam_fn is None or not os.path.exists(args.tumor_bam_fn):
                sys.exit("[ERROR] Pls input --tumor_bam_fn for calculation")
            if args.tumor_bam_fn.lower().endswith(".cram"):
                sys.exit("compare_vcf: CRAM input is not supported; give a BAM with its .bai")
            try:
                result_dict = cal_af(args, truth_variant_dict, input_variant_dict)
            except RuntimeError as e:
                sys.exit("compare_vcf: %s" % e)
            if result_dict is None:
                sys.exit("compare_vcf: --output_path sends cal_af's rows to that file and the reference fails on what is left; drop it "
                         "under --min_af")
        else:
            result_dict = OrderedDict()
            for row in open(args.low_af_path).readlines():
                row = row.rstrip().split(" ")
                if len(row) < 4:
                    sys.exit("compare_vcf: --low_af_path: a row with fewer than four columns")
                ctg, pos, tumor_cov, tumor_alt, *hap_info = row
                result_dict[ctg, int(pos)] = ctg, pos, tumor_cov, tumor_alt, hap_info
        for v in result_dict.values():
            ctg, pos, tumor_cov, tumor_alt = v[:4]
            key = int(pos) if ctg_name is not None else (ctg, int(pos))
            if int(tumor_alt) == 0 or int(tumor_cov) == 0:
                low_af_truth.add(key)
            elif int(tumor_alt) / float(tumor_cov) < args.min_af or int(tumor_alt) <= args.min_alt_coverage:
                low_af_truth.add(key)
        for k in list(input_variant_dict.keys()):
            if input_variant_dict[k].af is None:
                sys.exit("compare_vcf: --min_af: the input row of {} has neither AF nor VAF".format(k))
            if float(input_variant_dict[k].af) < args.min_af:
                del input_variant_dict[k]

    validate_phase = 0
    if args.validate_phase_only is not None:
        try:
            validate_phase = int(args.validate_phase_only)
        except ValueError:
            sys.exit("compare_vcf: --validate_phase_only {} is no integer".format(args.validate_phase_only))
        if args.phase_output is not None:
            phase_dict = OrderedDict()
            for item in open(args.phase_output).readlines():
                row = item.rstrip().split(" ")
                if len(row) != 10:
                    sys.exit("compare_vcf: --phase_output: a row with {} columns, not ctg pos depth alt and six haplotype counts".format(len(row)))
                ctg, pos, tumor_cov, tumor_alt, *hap_info = row
                phase_dict[ctg, int(pos)] = (ctg, pos, tumor_cov, tumor_alt, hap_info)
        elif result_dict is None:
            sys.exit("compare_vcf: --validate_phase_only needs --phase_output (the reference fails on a name it never set)")
        else:
            phase_dict = result_dict
        for item in phase_dict.values():
            if len(item) != 5 or len(item[4]) != 6:
                sys.exit("compare_vcf: --validate_phase_only: a row without its six haplotype counts")
            ctg, pos, tumor_cov, tumor_alt, hap_info = item
            hp0, hp1, hp2, all_hp0, all_hp1, all_hp2 = [int(i) for i in hap_info]
            key = int(pos) if ctg_name is not None else (ctg, int(pos))
            if key in input_variant_dict:
                continue
            phaseable = all_hp1 * all_hp2 > 0 and hp1 * hp2 == 0 and (hp1 > args.min_alt_coverage or hp2 > args.min_alt_coverage)
            if (validate_phase == 1 and not phaseable) or (validate_phase == 2 and phaseable):
                low_af_truth.add(key)

    # ---- the two dicts as arrays, the four loops and the sweeps as one call
    contigs, alleles = OrderedDict(), {}
    with_h = args.validate_phase_only is not None
    tin = _table(input_variant_dict, contigs, alleles, ctg_name, low_af_truth, with_h)
    ttr = _table(truth_variant_dict, contigs, alleles, ctg_name, low_af_truth, False)
    if with_h:
        # the input-dict half of the gate is rule 4 of the call; its counts are printed here
        phasable_count = int(np.count_nonzero(tin["flags"] & H))
        print("[INFO] Fail or non-phasable:", len(input_variant_dict) - phasable_count, 'Low ALT base phase count :', 0, "Phasable:", phasable_count)
    trees = [fp_bed_tree] + strat_bed_tree_list
    for t in trees:
        for name in t.intervals:
            contigs.setdefault(name, len(contigs))
    cutoffs, roc_cutoffs = [], []
    finite = tin["qual"][np.isfinite(tin["qual"])]
    if args.output_best_f1_score:
        # a superset of the reference's list: fp_set and tp_set are not known before the call
        cutoffs = np.unique(np.trunc(finite)) if args.use_int_cut_off else np.array([item / 100.0 for item in range(0, 101)])
    if args.roc_fn:
        roc_cutoffs = np.unique(finite)
    stats = {}
    try:
        r = compare_calls(tin, ttr, pack_beds(trees, contigs), len(contigs), benchmark_indel, high_confident_only, args.skip_genotyping,
                          validate_phase if validate_phase in (1, 2) else 0, cutoffs, roc_cutoffs, where=where, host_threads=args.threads or 0,
                          stats=stats)
    except RuntimeError as e:
        sys.exit("compare_vcf: %s" % e)
    c = r["counters"]
    in_keys, tr_keys = list(input_variant_dict.keys()), list(truth_variant_dict.keys())
    members = lambda keys, sets, bit: [k for k, s in zip(keys, sets.tolist()) if s & bit]
    fp_keys, tp_keys = members(in_keys, r["input_sets"], FP), members(in_keys, r["input_sets"], TP)
    fp_set, tp_set = set(fp_keys), set(tp_keys)
    fn_set = set(members(in_keys, r["input_sets"], FN)) | set(members(tr_keys, r["truth_sets"], FN))
    fp_fn_set = set(members(in_keys, r["input_sets"], FP_FN))
    input_left, truth_left = set(members(in_keys, r["input_sets"], KEPT)), set(members(tr_keys, r["truth_sets"], KEPT))
    tp_snv, tp_ins, tp_del, fp_snv, fp_ins, fp_del, fn_snv, fn_ins, fn_del = (c[k] for k in COUNTERS[:9])

    output_file = open(args.output_fn, "w") if args.output_fn else None
    if not args.skip_genotyping:
        print('[INFO] Genotype mismatch count/Total fp_fn count: {}/{}'.format(c["gt_mismatch"], len(fp_fn_set)))
    tp_indel, fp_indel, fn_indel = tp_ins + tp_del, fp_ins + fp_del, fn_ins + fn_del
    snv_pre, snv_rec, snv_f1 = cal_metrics(tp=tp_snv, fp=fp_snv, fn=fn_snv)
    print("\n")
    # the reference's third count is of records the first loop has deleted already: always 0
    print("[INFO] Total input records: {}, truth records: {}, records out of BED:{}".format(c["n_input_left"], c["n_truth_left"], 0))
    print(''.join([item.ljust(13) for item in ["Type", 'Precision', 'Recall', "F1-score", 'TP', 'FP', 'FN', ""]]), file=output_file)
    print(''.join([str(item).ljust(13) for item in ["SNV", snv_pre, snv_rec, snv_f1, tp_snv, fp_snv, fn_snv, ""]]), file=output_file)
    if benchmark_indel:
        indel_pre, indel_rec, indel_f1 = cal_metrics(tp=tp_indel, fp=fp_indel, fn=fn_indel)
        ins_pre, ins_rec, ins_f1 = cal_metrics(tp=tp_ins, fp=fp_ins, fn=fn_ins)
        del_pre, del_rec, del_f1 = cal_metrics(tp=tp_del, fp=fp_del, fn=fn_del)
        for row in (["INDEL", indel_pre, indel_rec, indel_f1, tp_indel, fp_indel, fn_indel, tp_indel + fn_indel],
                    ["INS", ins_pre, ins_rec, ins_f1, tp_ins, fp_ins, fn_ins, tp_ins + fn_ins],
                    ["DEL", del_pre, del_rec, del_f1, tp_del, fp_del, fn_del, tp_del + fn_del]):
            print(''.join([str(item).ljust(13) for item in row]), file=output_file)

    fmt = lambda row: ''.join([str(item).ljust(13) if idx >= 4 or idx == 0 else ('%.4f' % item).ljust(13) for idx, item in enumerate(row)])
    if args.output_best_f1_score:
        fp_quals = [_as_float(input_variant_dict[k].qual) for k in fp_keys]
        tp_quals = [_as_float(input_variant_dict[k].qual) for k in tp_keys]
        if any(q is None for q in fp_quals + tp_quals):
            sys.exit("compare_vcf: --output_best_f1_score: a call of the sweep has no QUAL")
        if args.use_int_cut_off:
            try:
                qual_list = set([int(q) for q in fp_quals + tp_quals])
            except (ValueError, OverflowError):
                sys.exit("compare_vcf: --output_best_f1_score: a QUAL that is not finite")
        else:
            qual_list = [item / 100.0 for item in range(0, 101)]
        counts = {float(q): (int(f), int(t)) for q, (f, t) in zip(np.asarray(cutoffs).tolist(), r["sweep"].tolist())}
        results = []
        for qual in qual_list:
            n_fp, n_tp = counts[float(qual)]
            n_fn = len(fn_set) + len(tp_quals) - n_tp
            pre, rec, f1 = cal_metrics(tp=n_tp, fp=n_fp, fn=n_fn)
            results.append([qual, pre, rec, f1, n_tp, n_fp, n_fn, n_tp + n_fn])
        results = sorted(results, key=lambda x: x[3], reverse=True)
        if not results:
            sys.exit("compare_vcf: --output_best_f1_score: no call to take a cut-off from")
        best_match = results[0].copy()
        best_match[0] = 'SNV(Best F1)'
        print(fmt(best_match), file=output_file)
        if args.debug:
            print("")
            for result in results:
                print(fmt(result), file=output_file)

    if args.roc_fn:
        try:
            fp_dict = dict([(key, float(input_variant_dict[key].qual)) for key in fp_set])
            tp_dict = dict([(key, float(input_variant_dict[key].qual)) for key in tp_set])
        except (TypeError, ValueError):
            sys.exit("compare_vcf: --roc_fn: a call of the sweep has no QUAL")
        qual_list = sorted([float(qual) for qual in fp_dict.values()] + [qual for qual in tp_dict.values()], reverse=True)
        counts = {float(q): (int(f), int(t)) for q, (f, t) in zip(np.asarray(roc_cutoffs).tolist(), r["roc_sweep"].tolist())}
        tp_count = len(tp_set)
        with open(args.roc_fn, "w") as roc_fn:
            for qual_cut_off in set(qual_list):
                pass_fp_count, pass_tp_count = counts[qual_cut_off] if qual_cut_off == qual_cut_off else (0, 0)
                fn_count = tp_count - pass_tp_count + fn_snv
                tmp_pre, tmp_rec, tmp_f1 = cal_metrics(tp=pass_tp_count, fp=pass_fp_count, fn=fn_count)
                roc_fn.write('\t'.join([str(round(item, 4)) for item in [qual_cut_off, tmp_pre, tmp_rec, tmp_f1]]) + '\n')

    if args.log_som is not None and os.path.exists(args.log_som):
        for row in open(args.log_som).readlines():
            if 'SNVs' not in row:
                continue
            columns = row.rstrip().split(',')
            tp, fp, fn = [float(item) for item in columns[4:7]]
            if int(tp_snv) != int(tp):
                print("True positives not match")
            if int(fp_snv) != int(fp):
                print("False positives not match")
            if int(fn_snv) != int(fn):
                print("False negatives not match")

    if args.output_dir is not None:
        os.makedirs(args.output_dir, exist_ok=True)
        for vcf_type, variant_set in zip(['fp', 'fn', 'fp_fn', 'tp'], [fp_set, fn_set, fp_fn_set, tp_set]):
            if ctg_name is None and any(key[0] not in major_contigs_order for key in variant_set):
                sys.exit("compare_vcf: --output_dir without --ctg_name sorts by the reference's list of chr1 .. chrY / 1 .. Y, and a key is on "
                         "another contig")
            variant_list = sorted(variant_set, key=sort_key) if ctg_name is None else sorted(variant_set)
            with open(os.path.join(args.output_dir, '{}.vcf'.format(vcf_type)), "w") as vcf_writer:     # VcfWriter(write_header=False): the rows
                for key in variant_list:
                    if key in input_left:
                        vcf_writer.write(input_variant_dict[key].row_str)
                    elif key in truth_left:
                        vcf_writer.write(truth_variant_dict[key].row_str)
    if output_file is not None:
        output_file.close()
    return None


def build_parser():
    """every option of the reference's parser (src/compare_vcf.py:541-651) at its arity, type and default, and --where / --bai_fn"""
    ap = argparse.ArgumentParser(prog="compare_vcf", description="Compare input VCF with truth VCF")
    ap.add_argument("--bed_fn", type=str, default=None, help="High confident BED region for benchmarking")
    ap.add_argument("--input_vcf_fn", type=str, default=None, help="Input VCF filename")
    ap.add_argument("--truth_vcf_fn", type=str, default=None, help="Truth VCF filename")
    ap.add_argument("--ctg_name", type=str, default=None, help="The name of the contig to be processed")
    ap.add_argument("--ctg_start", type=int, default=None, help="The 1-based starting position of the sequence to be processed")
    ap.add_argument("--ctg_end", type=int, default=None, help="The 1-based ending position of the sequence to be processed")
    ap.add_argument("--output_dir", type=str, default=None, help="Output directory: fp.vcf, fn.vcf, fp_fn.vcf, tp.vcf")
    ap.add_argument("--input_filter_tag", type=str_none, default=None, help="Filter variants with tag from the input VCF")
    ap.add_argument("--truth_filter_tag", type=str_none, default=None, help="Filter variants with tag from the truth VCF")
    ap.add_argument("--tumor_bam_fn", type=str, default=None, help="Sorted tumor BAM file input, for --min_af")
    ap.add_argument("--threads", type=int, default=8, help="Host threads of --where host")
    ap.add_argument("--min_af", type=float, default=None, help="EXPERIMENTAL: Minimum VAF for a variant to be included in benchmarking")
    ap.add_argument("--min_alt_coverage", type=int, default=2, help="EXPERIMENTAL: Minimum alt base count for a variant to be included in benchmarking")
    ap.add_argument("--strat_bed_fn", type=str, default=None, help="EXPERIMENTAL: Genome stratifications v2 bed regions, comma-separated")
    ap.add_argument("--output_fn", type=str, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--low_af_path", type=str, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--high_confident_only", type=str, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--skip_genotyping", type=str2bool, default=True, help="Skip calculating VCF genotype")
    ap.add_argument("--roc_fn", type=str, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--log_som", type=str, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--output_best_f1_score", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--use_int_cut_off", type=str2bool, default=True, help=argparse.SUPPRESS)
    ap.add_argument("--benchmark_indel", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--output_path", type=str, default=None, help=argparse.SUPPRESS)          # cal_af reads it (see the module's quirks)
    ap.add_argument("--phase_output", type=str, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--validate_phase_only", type=str_none, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--min_qual", type=float, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--max_qual", type=float, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--debug", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--where", choices=("device", "host"), default=None, help="default: device when a GPU is present")
    ap.add_argument("--bai_fn", type=str, default=None, help="index of --tumor_bam_fn; default: <tumor_bam_fn>.bai")
    # parsed by the reference and never read: --discard_fn_out_of_fp_bed is copied into a local nothing looks at; --samtools is read by the
    # reference's cal_af only, which is not run here
    add_ignored(ap, platform="str", ref_fn="str", samtools="str", min_coverage="int", discard_fn_out_of_fp_bed="str")
    return ap


def main(argv=None):
    compare_vcf(build_parser().parse_args(argv))
    return 0


if __name__ == "__main__":
    main(sys.argv[1:])
