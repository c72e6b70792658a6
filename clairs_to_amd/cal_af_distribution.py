"""The reference's src/cal_af_distribution.py without samtools: per truth variant the depth, the ALT count and the per-haplotype counts
the tumour BAM shows - the AF half of its compare_vcf step (src/compare_vcf.py:151 calls cal_af) and a command of its own.  The reference
starts one `samtools mpileup -r ctg:pos-pos` per variant and parses that row character by character; here all variants of a contig are
one cto_af_tallies call (csrc/aftally.hip: the rules, the device path; csrc/bam.cpp: the host path).  PARITY UNPINNED against samtools
(DESIGN.md); what the reference makes of a pile-up row is pinned by tests/golden/cal_af.json.gz.

    python -m clairs_to_amd cal_af_distribution --tumor_bam_fn BAM --truth_vcf_fn TRUTH --input_vcf_fn CALLS [--ctg_name CTG]
        [--truth_filter_tag PASS] [--input_filter_tag PASS] [--phase_output True] --output_path OUT [--where device|host] [--bai_fn BAI]

Quirks kept (src/cal_af_distribution.py:44-115, 137-210): rows of truth variants the input VCF also holds come first, as
`ctg pos DP round(AF * DP)`; the pile-up rows follow in truth order, `ctg pos depth alt h0 h1 h2 a0 a1 a2`; entry i of a column is
paired with HP value i although a reference skip has an HP value and no entry; HP 12 raises."""
import argparse
import ctypes as C
import gzip
import os
import sys
from collections import OrderedDict

import numpy as np

from ._cli import add_ignored, str2bool

MIN_MQ = 20               # shared/param.py: min_mq - the reference passes this, not --min_mq
EXCL_FLAGS = 2316
MAX_DEPTH = 8000          # samtools mpileup's default -d: every variant is a run of its own
KIND_SNV, KIND_INS, KIND_DEL, KIND_NEVER = 0, 1, 2, 3


def _default_where():
    import torch
    return "device" if torch.cuda.is_available() else "host"


class Variant(object):
    """what cal_af and compare_vcf read of shared/utils.py:Position"""
    __slots__ = ("ctg_name", "pos", "reference_bases", "alternate_bases", "row_str", "genotype", "qual", "af")

    def __init__(self, ctg_name, pos, ref_base, alt_base, row_str, genotype=None, qual=None, af=None):
        self.ctg_name, self.pos, self.reference_bases, self.row_str = ctg_name, pos, ref_base, row_str
        self.alternate_bases = [alt_base] if "," not in alt_base else alt_base.split(",")
        self.genotype, self.qual, self.af = genotype, qual, af


def read_vcf(vcf_fn, ctg_name=None, filter_tag=None, ctg_start=None, ctg_end=None, skip_genotype=False, keep_af=False, min_qual=None, max_qual=None,
             discard_indel=False):
    """shared/vcf.py:238-352, VcfReader(vcf_fn, ctg_name, show_ref=False, keep_row_str=True, filter_tag, ...).read_vcf() -> variant_dict: key = POS
    when ctg_name is one name, (CHROM, POS) otherwise; a repeated key keeps its first place and its last row; 0/0 rows are dropped unless
    skip_genotype, a genotype that does not parse is kept as [-1, -1]; the `*` ALT rule of :312-320; plain or gzip input (the reference pipes every
    file through `gzip -fdc`).  compare_vcf's options: rows outside ctg_start .. ctg_end (both given) are dropped; discard_indel drops a row whose
    REF or whole ALT string is longer than one letter (a multi-allelic SNV row too); min_qual / max_qual drop by float(QUAL), and a QUAL they
    cannot parse becomes None; keep_af stores AF (or VAF) of column 10 by column 9's index, None without either."""
    out = OrderedDict()
    if vcf_fn is None or not os.path.exists(vcf_fn):
        return out
    with open(vcf_fn, "rb") as f:
        gz = f.read(2) == b"\x1f\x8b"
    if ctg_name is None:
        only, tuple_keys = None, True
    elif "," in ctg_name:
        only, tuple_keys = frozenset(x.strip() for x in ctg_name.split(",") if x.strip()), True
    else:
        only, tuple_keys = frozenset([ctg_name]), False
    allowed = None if filter_tag is None else filter_tag.split(",")
    in_region = ctg_start is not None and ctg_end is not None
    header_last_column = []
    with (gzip.open(vcf_fn, "rt") if gz else open(vcf_fn)) as fo:
        for row in fo:
            columns = row.strip().split()
            if columns[0][0] == "#":
                header_last_column = columns
                continue
            tumor_in_last = bool(header_last_column) and header_last_column[-1].rstrip().lower() == "tumor"
            chromosome, position = columns[0], columns[1]
            if only is not None and chromosome not in only:
                continue
            if in_region and not (ctg_start <= int(position) <= ctg_end):
                continue
            flt = columns[6] if len(columns) >= 7 else None
            if allowed is not None and flt not in allowed:
                continue
            reference, alternate = columns[3], columns[4]
            if discard_indel and (len(reference) > 1 or len(alternate) > 1):
                continue
            try:
                qual = columns[5] if len(columns) > 5 else None
                if min_qual is not None and float(qual) < min_qual:
                    continue
                if max_qual is not None and float(qual) > max_qual:
                    continue
            except Exception:
                qual = None
            last_column = columns[-2] if tumor_in_last else columns[-1]
            genotype = last_column.split(":")[0].replace("/", "|").replace(".", "0").split("|")
            try:
                g1, g2 = genotype
                if int(g1) > int(g2):
                    g1, g2 = g2, g1
                if "*" in alternate:
                    alts = alternate.split(",")
                    if int(g1) + int(g2) != 3 or len(alts) != 2:
                        print("error with variant representation")
                        continue
                    alternate = "".join(a for a in alts if a != "*")
                    g1, g2 = "0", "1"
            except Exception:
                g1 = g2 = -1
            af = None
            if keep_af:
                tag_list = columns[8].split(":")
                if "AF" in tag_list or "VAF" in tag_list:
                    af = float(columns[9].split(":")[tag_list.index("AF") if "AF" in tag_list else tag_list.index("VAF")])
            position = int(position)
            if g1 == "0" and g2 == "0" and not skip_genotype:
                continue
            out[(chromosome, position) if tuple_keys else position] = Variant(chromosome, position, reference, alternate, row, [int(g1), int(g2)], qual, af)
    return out


def parser_info(row):
    """src/cal_af_distribution.py:125-134: ctg, pos (as text), DP and round(AF * DP) of a call's own row"""
    columns = row.split("\t")
    info_list = columns[8].split(":")
    fmt = columns[9].split(":")
    tumor_depth = int(fmt[info_list.index("DP")])
    return columns[0], columns[1], tumor_depth, round(float(fmt[info_list.index("AF")]) * tumor_depth)


def allele_of(ref_base, alt_base):
    """(kind, letter, del_len, inserted bytes): the entry of a pile-up column that counts as ALT (src/cal_af_distribution.py:93-98), for
    cto_af_tallies.  An entry is one of A C G T N, with `+SEQ` or `-N..N` behind it, or `*`; an allele no entry can equal is KIND_NEVER."""
    alt = alt_base.upper()
    if len(ref_base) == 1 and len(alt) > 1:
        if alt[0] in "ACGTN" and alt[1:].isalpha():               # inserted bases print as letters: nothing else can be equal
            return KIND_INS, alt[0], 0, alt[1:].encode()
    elif len(ref_base) > 1 and len(alt) == 1:
        if ref_base[0].upper() in "ACGTN":
            return KIND_DEL, ref_base[0].upper(), len(ref_base) - 1, b""
    elif len(alt) == 1 and alt in "ACGTN":
        return KIND_SNV, alt, 0, b""
    return KIND_NEVER, "N", 0, b""


def tally(bam, ctg, loci, alleles, min_mq=MIN_MQ, excl_flags=EXCL_FLAGS, max_depth=MAX_DEPTH, with_hp=True, where="device", bai=None,
          host_threads=0, stats=None):
    """int32 [n, 8] - depth, alt, h0 h1 h2, a0 a1 a2 - at the 1-based `loci` (strictly ascending) of contig `ctg`; alleles[i] =
    (kind, letter, del_len, inserted bytes) as allele_of gives it.  where: "device" (HIP kernels on the current stream) or "host".
    stats: a dict that receives the call's cto_af_stats.  An entry paired with HP 12 raises, as the reference does."""
    from ._lib import AfStats, check, lib
    if where not in ("device", "host"):
        raise ValueError("where must be 'device' or 'host'")
    pos = np.ascontiguousarray(loci, dtype=np.int32)
    n = len(pos)
    if len(alleles) != n:
        raise ValueError("one allele per locus")
    kind = np.array([a[0] for a in alleles], dtype=np.uint8)
    base = np.frombuffer("".join(a[1] for a in alleles).encode(), dtype=np.uint8) if n else np.zeros(0, dtype=np.uint8)
    del_len = np.array([a[2] for a in alleles], dtype=np.int32)
    ins_off = np.zeros(n + 1, dtype=np.int64)
    ins_off[1:] = np.cumsum([len(a[3]) for a in alleles])
    ins = b"".join(a[3] for a in alleles) + b"\0"
    out = np.zeros((n, 8), dtype=np.int32)
    st = AfStats()
    stream = None
    if where == "device":
        from ._lib import current_stream_ptr
        stream = C.c_void_p(current_stream_ptr())
    check(lib.cto_af_tallies(str(bam).encode(), str(bai).encode() if bai else None, ctg.encode(), pos.ctypes.data, n, kind.ctypes.data,
                             base.ctypes.data, del_len.ctypes.data, C.cast(C.c_char_p(ins), C.c_void_p), ins_off.ctypes.data, int(min_mq),
                             int(excl_flags), int(max_depth), 1 if with_hp else 0, 1 if where == "device" else 0, int(host_threads), stream,
                             out.ctypes.data, C.byref(st)))
    if stats is not None:
        for name, _ in AfStats._fields_:
            stats[name] = stats.get(name, 0) + getattr(st, name)
    return out


def pileup_rows(args, variants, where, stats=None):
    """extract_base (src/cal_af_distribution.py:77-115) for every variant, in order: [ctg, pos, depth, alt, "h0 h1 h2", "a0 a1 a2"]"""
    by_ctg = OrderedDict()                                        # contig -> {pos: [variant index]}
    for i, v in enumerate(variants):
        by_ctg.setdefault(v.ctg_name, {}).setdefault(v.pos, []).append(i)
    rows = [None] * len(variants)
    for ctg, at in by_ctg.items():
        loci = sorted(at)
        if loci[0] < 1 or loci[-1] >= 2 ** 31:
            sys.exit("cal_af_distribution: position out of range on %s" % ctg)
        # a dict a caller built itself may hold two variants at one position: cto_af_tallies takes a position once, so they go in turns
        for turn in range(max(len(x) for x in at.values())):
            sub = [p for p in loci if len(at[p]) > turn]
            idx = [at[p][turn] for p in sub]
            alleles = [allele_of(variants[i].reference_bases, variants[i].alternate_bases[0]) for i in idx]
            t = tally(args.tumor_bam_fn, ctg, sub, alleles, with_hp=bool(args.phase_output), where=where, bai=getattr(args, "bai_fn", None),
                      host_threads=getattr(args, "threads", 0) or 0, stats=stats)
            for i, c in zip(idx, t):
                rows[i] = [ctg, variants[i].pos, int(c[0]), int(c[1]), "%d %d %d" % tuple(c[2:5]), "%d %d %d" % tuple(c[5:8])]
    return rows


def cal_af(args, truth_variant_dict=None, input_variant_dict=None, stats=None):
    """src/cal_af_distribution.py:137-210.  With --output_path the reference's file is written (None is returned); without it the
    reference's results_dict comes back, with the same keys and tuples."""
    ctg_name = args.ctg_name
    output_path = args.output_path
    if truth_variant_dict is None:
        truth_variant_dict = read_vcf(args.truth_vcf_fn, ctg_name, args.truth_filter_tag)
    if input_variant_dict is None:
        input_variant_dict = read_vcf(args.input_vcf_fn, ctg_name, args.input_filter_tag)
    where = getattr(args, "where", None) or _default_where()
    results_dict = OrderedDict()
    variant_dict = OrderedDict()
    output_file = open(output_path, "w") if output_path is not None else None
    try:
        for k, v in truth_variant_dict.items():
            if k not in input_variant_dict:
                variant_dict[k] = v
            else:
                result = parser_info(input_variant_dict[k].row_str)
                if output_file is not None:
                    output_file.write(" ".join(str(item) for item in result) + "\n")
                else:
                    results_dict[k if args.ctg_name is None else (args.ctg_name, k)] = result
        print("[INFO] Total truth need to calculate AF: {}".format(len(variant_dict)))
        for result in pileup_rows(args, list(variant_dict.values()), where, stats=stats):
            ctg, pos, depth, alt_depth, hap_list, all_hap_list = result
            results_dict[(ctg, int(pos))] = ctg, pos, depth, alt_depth, hap_list, all_hap_list
            if output_file is not None:
                output_file.write(" ".join(str(item) for item in result) + "\n")
    finally:
        if output_file is not None:
            output_file.close()
    if output_path is not None:
        return None
    return results_dict


def build_parser():
    """every option of the reference's parser (src/cal_af_distribution.py:213-254) at its arity, and --where / --bai_fn"""
    ap = argparse.ArgumentParser(prog="cal_af_distribution", description="Calculate AF distribution in tumor BAM")
    ap.add_argument("--tumor_bam_fn", type=str, default=None, help="Sorted tumor BAM file input, required")
    ap.add_argument("--input_vcf_fn", type=str, default=None, help="Input VCF filename")
    ap.add_argument("--truth_vcf_fn", type=str, default=None, help="Input truth VCF filename")
    ap.add_argument("--input_filter_tag", type=str, default=None, help="Filter variants with tag from the input VCF")
    ap.add_argument("--truth_filter_tag", type=str, default=None, help="Filter variants with tag from the truth VCF")
    ap.add_argument("--ctg_name", type=str, default=None, help="The name of the sequence to be processed; all contigs when not given")
    ap.add_argument("--output_path", type=str, default=None, help="Output filename; without it cal_af returns its rows")
    ap.add_argument("--threads", type=int, default=4, help="Host threads of --where host")
    ap.add_argument("--phase_output", type=str2bool, default=True, help="Output phasing INFO")
    ap.add_argument("--where", choices=("device", "host"), default=None, help="default: device when a GPU is present")
    ap.add_argument("--bai_fn", type=str, default=None, help="index of --tumor_bam_fn; default: <tumor_bam_fn>.bai")
    # --samtools is not run; --min_mq, --min_bq and --min_bq_cut are parsed by the reference and never read (it passes shared/param.py's
    # min_mq = 20 and min_bq = 0 to samtools, and get_base_list is called without args)
    add_ignored(ap, samtools="str", min_mq="int", min_bq="int", min_bq_cut="int")
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if not args.tumor_bam_fn:
        sys.exit("cal_af_distribution: --tumor_bam_fn is required")
    if args.tumor_bam_fn.lower().endswith(".cram"):
        sys.exit("cal_af_distribution: CRAM input is not supported; give a BAM with its .bai")
    try:
        cal_af(args)
    except RuntimeError as e:
        sys.exit("cal_af_distribution: %s" % e)
    return 0


if __name__ == "__main__":
    main(sys.argv[1:])
