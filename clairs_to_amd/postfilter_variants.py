"""Drop-in counterpart of `clairs_to.py postfilter_variants` (reference: src/postfilter_variants.py; STEP 4-2 / 8-2 of run_clairs_to for
short reads): tags the PASS calls of the realignment VCF with the short-read hard filters (ReadStartEnd, VariantCluster,
StrandBias, LowSeqEntropy) and the strand-bias p-value `SB`, from the tumour BAM.

Same inputs, options, PF_INFO_* file, stdout and output VCF as the reference.  What differs is how the work is done: the reference starts
one `pypy3` process and one `samtools mpileup` per call under GNU parallel (or, in its chunk mode, one Python dict-of-dicts pass per <= 256
calls); here the calls of a contig are cut into mpileup jobs, producer threads fetch and pack each job's eight-column text
(cto_postfilter_pack, csrc/postfilter.hip), and the packed jobs go in batches to ONE kernel launch each (cto_postfilter_windows: a workgroup
per call walks the +-flanking window's read-bases) while the producers fetch the next ones.  Python keeps what decides printed digits in the
reference: Fisher's test on the returned 2x2 table (exact integers, then the reference's float loop), the 33-base sequence entropy of indel
calls, and the float thresholds on the returned integers, all evaluated by the same interpreter arithmetic as the reference.  There is no
CPU fallback: without the library or a device the module raises.
"""
import bisect
import ctypes as C
import math
import os
import shlex
import subprocess
import sys
from argparse import ArgumentParser
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from ._cli import add_ignored, str2bool, str_none
from ._lib import lib, check
from .fasta import read_region
from .haplotype_filtering import fisher_exact_two_sided, header_up_to_last_format, partition_jobs, read_vcf

MAX_SITES_PER_JOB, MAX_SPAN_PER_JOB = 256, 50000            # postfilter_variants.py:182-183
JOBS_PER_LAUNCH = 16                                        # packed jobs handed to one kernel launch
NO_OF_POSITIONS, FLANKING_BASE_NUM = 33, 16                 # shared/param.py no_of_positions, flankingBaseNum
SEQUENCE_ENTROPY_THRESHOLD = 0.9                            # :21
MODULE_FLANKING = 100                                       # :22
BASE2NUM = dict(zip("ACGTURYSWKMBDHVN", (0, 1, 2, 3, 3, 0, 1, 1, 0, 2, 0, 1, 0, 0, 0, 0)))       # shared/utils.py:18-21
OUT_FIELDS = ("n_alt", "n_rse", "match_count", "ins_length", "depth", "a0", "r0", "a1", "r1", "host_path")


# ------------------------------------------------------------------------------------------ per-call scalars kept in Python
def sequence_entropy(sequence, entropy_window=NO_OF_POSITIONS, kmer=5):
    """calculate_sequence_entropy (:92-135): the 5-mer entropy of the last `entropy_window` k-mer starts, in the reference's order of
    floating-point operations"""
    counts = [0] * (entropy_window + 2)
    counts[0] = entropy_window
    entropy = [0.0] * (entropy_window + 2)
    for i in range(1, entropy_window + 2):
        e = 1.0 / entropy_window * i
        entropy[i] = e * math.log(e)
    entropy_mul = -1 / math.log(entropy_window)
    hash_counts = [0] * (1 << (2 * kmer))
    mask = ~((-1) << (2 * kmer))
    suffix = prefix = 0
    i, i2, total = 0, -entropy_window, 0.0
    while i2 < len(sequence):
        if i < len(sequence):
            suffix = ((suffix << 2) | BASE2NUM[sequence[i]]) & mask
            counts[hash_counts[suffix]] -= 1
            total -= entropy[hash_counts[suffix]]
            hash_counts[suffix] += 1
            counts[hash_counts[suffix]] += 1
            total += entropy[hash_counts[suffix]]
        if i2 >= 0 and i < len(sequence):
            prefix = ((prefix << 2) | BASE2NUM[sequence[i2]]) & mask
            counts[hash_counts[prefix]] -= 1
            total -= entropy[hash_counts[prefix]]
            hash_counts[prefix] -= 1
            counts[hash_counts[prefix]] += 1
            total += entropy[hash_counts[prefix]]
        i += 1
        i2 += 1
    return total * entropy_mul


def site_entropy(ref_seq_site):
    """sqeuence_entropy_from (:138-144): the slice is taken at the module's `flanking = 100` (:22) whatever --flanking says, and not at the
    call's offset in a window clipped at position 1 - with --flanking 50 it is the window's last 18 bases"""
    return sequence_entropy(ref_seq_site[MODULE_FLANKING - FLANKING_BASE_NUM: MODULE_FLANKING + FLANKING_BASE_NUM + 1])


def call_kind(ref_base, alt_base):
    """0 SNV, 1 insertion, 2 deletion, 3 neither (:372-374)"""
    if len(ref_base) == 1 and len(alt_base) == 1:
        return 0
    if len(ref_base) == 1 and len(alt_base) > 1:
        return 1
    if len(ref_base) > 1 and len(alt_base) == 1:
        return 2
    return 3


def finalize_line(ctg, pos, ref_base, alt_base, counts, ref_seq_site, flanking, disable_rse, max_co_exist_read_num):
    """_postfilter_finalize_line (:286-365) from the integers of cto_postfilter_windows -> the reference's per-call output line"""
    n_alt, n_rse, match_count, ins_length, depth, a0, r0, a1, r1 = (int(v) for v in counts[:9])
    pass_rse = not (not disable_rse and n_rse >= 0.3 * n_alt)
    depth = depth if depth > 0 else 1
    pass_co_exist = not (match_count >= max_co_exist_read_num or ins_length / depth > 3)
    p_value = fisher_exact_two_sided(a0, r0, a1, r1)
    pass_sb = not p_value < 0.001
    pass_entropy = True
    if not (len(ref_base) == 1 and len(alt_base) == 1):
        pass_entropy = not site_entropy(ref_seq_site) < SEQUENCE_ENTROPY_THRESHOLD
    pass_all = pass_rse and pass_co_exist and pass_sb and pass_entropy
    return " ".join([ctg, str(pos), str(pass_all), str(pass_rse), str(pass_co_exist), str(pass_sb), str(round(p_value, 5)), str(pass_entropy)])


# ------------------------------------------------------------------------------------------ the C calls
class PackedJob(object):
    """one mpileup job's text packed for the device (cto_postfilter_pack); freed with the object"""

    def __init__(self, text, ref_seq, region_lo, flanking):
        tb = text if isinstance(text, (bytes, bytearray)) else text.encode()
        rb = ref_seq.encode() if isinstance(ref_seq, str) else ref_seq
        self.handle = C.c_void_p()
        tarr = np.frombuffer(tb, dtype=np.uint8) if len(tb) else np.zeros(1, dtype=np.uint8)
        check(lib.cto_postfilter_pack(tarr.ctypes.data, len(tb), rb, int(region_lo), len(rb), int(flanking), C.byref(self.handle)))

    def view(self):
        """the packed arrays as numpy copies, and the key / token strings (tests, tools)"""
        from ._lib import PfView
        v = PfView()
        check(lib.cto_postfilter_view_of(self.handle, C.byref(v)))
        arr = lambda p, n, t: np.ctypeslib.as_array(C.cast(p, C.POINTER(t)), shape=(n,)).copy() if n else np.zeros(0, dtype=t)
        out = dict(col_pos=arr(v.col_pos, v.n_cols, C.c_int32), col_off=arr(v.col_off, v.n_cols + 1, C.c_int64),
                   ent_tok=arr(v.ent_tok, v.n_names, C.c_uint32), ent_rid=arr(v.ent_rid, v.n_names, C.c_uint32),
                   col_tok_off=arr(v.col_tok_off, v.n_cols + 1, C.c_int64), tok_cnt=arr(v.tok_cnt, v.n_tokens, C.c_uint32),
                   tok_meta=arr(v.tok_meta, v.n_tokens, C.c_uint32), col_flags=arr(v.col_flags, v.n_cols, C.c_uint8))
        s = C.c_char_p()
        keys = []
        for k in range(v.n_keys):
            check(lib.cto_postfilter_key_string(self.handle, k, C.byref(s)))
            keys.append(s.value.decode())
        toks = []
        for c in range(v.n_cols):
            row = []
            for t in range(int(out["col_tok_off"][c + 1] - out["col_tok_off"][c])):
                check(lib.cto_postfilter_token_string(self.handle, c, t, C.byref(s)))
                row.append(s.value.decode())
            toks.append(row)
        out.update(keys=keys, tokens=toks)
        return out

    def __del__(self):
        if getattr(self, "handle", None):
            lib.cto_postfilter_free(self.handle)
            self.handle = None


def evaluate_windows(jobs, calls, max_id_range=0, want_kernel_ms=False):
    """jobs: [PackedJob]; calls: [(job index, pos, ref_base, alt_base)] -> int64 array [n, 10] (OUT_FIELDS) through ONE
    cto_postfilter_windows call (one kernel launch for all calls the device takes)"""
    n = len(calls)
    out = np.zeros((n, len(OUT_FIELDS)), dtype=np.int64)
    handles = (C.c_void_p * max(1, len(jobs)))(*[j.handle for j in jobs])
    cj = np.array([c[0] for c in calls], dtype=np.int32)
    cp = np.array([c[1] for c in calls], dtype=np.int32)
    ck = np.array([call_kind(c[2], c[3]) for c in calls], dtype=np.int32)
    cr = np.array([len(c[2]) for c in calls], dtype=np.int32)
    alts = [c[3].encode() for c in calls]
    off = np.zeros(n + 1, dtype=np.int64)
    if n:
        off[1:] = np.cumsum([len(a) for a in alts])
    blob = b"".join(alts) + b"\0"
    ms = C.c_double(0.0)
    check(lib.cto_postfilter_windows(len(jobs), handles, n, cj.ctypes.data, cp.ctypes.data, ck.ctypes.data, cr.ctypes.data, blob, off.ctypes.data,
                                     int(max_id_range), out.ctypes.data, C.byref(ms)))
    return (out, ms.value) if want_kernel_ms else out


# ------------------------------------------------------------------------------------------ mpileup text
def tumor_bam_of(args, contig):
    bam = args.tumor_bam_fn
    if not os.path.exists(bam):
        bam += contig + ".bam"                               # :466-467, :662-663
    return bam


def index_mpileup_file(fn):
    """`--mpileup_fn` read once: {contig: (sorted positions, rows)}"""
    index = {}
    with open(fn, "rb") as f:
        for row in f:
            c = row.split(b"\t", 2)
            if len(c) > 2:
                index.setdefault(c[0].decode(), []).append((int(c[1]), row))
    out = {}
    for ctg, rows in index.items():
        rows.sort(key=lambda r: r[0])
        out[ctg] = ([r[0] for r in rows], [r[1] for r in rows])
    return out


def mpileup_text(args, contig, lo, hi, prepared=None):
    """the eight-column text of one job: from `--mpileup_fn` (prepared = its index; rows outside [lo, hi] and of other contigs are dropped,
    what `-r` does) or the reference's own samtools command (:263-270)"""
    if prepared is not None:
        pos, rows = prepared.get(contig, ([], []))
        return b"".join(rows[bisect.bisect_left(pos, lo):bisect.bisect_right(pos, hi)])
    cmd = "{} mpileup --min-MQ {} --min-BQ {} --excl-flags 2316 -r {} --output-MQ --output-QNAME ".format(
        args.samtools, args.min_mq, args.min_bq, "{}:{}-{}".format(contig, lo, hi)) + tumor_bam_of(args, contig)
    res = subprocess.run(shlex.split(cmd), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if res.returncode != 0:           # the reference does not look (its calls then pass every read-level rule); say so, on stderr
        print("[WARNING] samtools mpileup failed (exit {}) for {}:{}-{}: {}".format(
            res.returncode, contig, lo, hi, res.stderr.decode(errors="replace").strip().replace("\n", " ")[:400]), file=sys.stderr, flush=True)
    return res.stdout


def produce_job(args, contig, lo, hi, flanking, prepared=None):
    """a producer thread's work for one job (outside the GIL: the samtools child, the C packer) -> (PackedJob, reference of [lo, hi])"""
    ref = read_region(args.ref_fn, contig, lo, hi) or ""
    return PackedJob(mpileup_text(args, contig, lo, hi, prepared), ref, lo, flanking), ref


def evaluate_calls(args, calls, threads=None, max_sites=MAX_SITES_PER_JOB, max_span=MAX_SPAN_PER_JOB, progress=None):
    """calls: [(contig, pos, ref_base, alt_base)] in the order the reference would report them -> {(contig, pos): output line}.
    Producer threads run ahead; the calling thread hands the packed jobs to the device, up to JOBS_PER_LAUNCH per call.
    progress(n): called after every launch with the number of calls evaluated so far."""
    flanking = args.flanking
    by_ctg = {}
    for c in calls:
        by_ctg.setdefault(c[0], []).append(c)
    jobs = []                                                  # (contig, lo, hi, [calls])
    for ctg, cs in by_ctg.items():
        at = {c[1]: c for c in cs}
        for lo, hi, ps in partition_jobs(at.keys(), flanking, max_sites, max_span):
            jobs.append((ctg, lo, hi, [at[p] for p in ps]))
    lines = {}
    threads = max(1, int(threads or 4))
    prepared = index_mpileup_file(args.mpileup_fn) if getattr(args, "mpileup_fn", None) else None

    def launch(batch):
        packed = [b[1][0] for b in batch]
        flat = [(k, c[1], c[2], c[3]) for k, (job, _) in enumerate(batch) for c in job[3]]
        out = evaluate_windows(packed, flat)
        i = 0
        for (ctg, lo, hi, cs), (_, ref) in batch:
            for c in cs:
                anchor = max(c[1] - flanking, 1)
                site = ref[anchor - lo: c[1] + flanking + 1 - lo + 1]           # :376-380
                lines[(ctg, c[1])] = finalize_line(ctg, c[1], c[2], c[3], out[i], site, flanking, args.disable_read_start_end_filtering,
                                                   args.min_alt_coverage)
                i += 1
        if progress is not None:
            progress(len(lines))

    with ThreadPoolExecutor(max_workers=min(threads, max(1, len(jobs)))) as ex:
        pending = deque((job, ex.submit(produce_job, args, job[0], job[1], job[2], flanking, prepared)) for job in jobs)
        while pending:
            # The batch is what is READY, in job order: wait for the next job, then add the ones behind it that are already packed.  The
            # device is never kept waiting for a fuller batch; when the producers are the slower side (samtools), launches are small
            # and cheap (one upload of the job's arrays, ~0.2 ms of kernel per few thousand calls), and the producers keep running meanwhile.
            batch = []
            while pending and len(batch) < JOBS_PER_LAUNCH and (not batch or pending[0][1].done()):
                job, fut = pending.popleft()
                batch.append((job, fut.result()))
            launch(batch)
    return lines


# ------------------------------------------------------------------------------------------ the stage
def postfilter_per_pos(args):
    """the reference's worker form (:460-483): one call described on the command line, one output line"""
    pos, ctg = args.pos, args.ctg_name
    lines = evaluate_calls(args, [(ctg, pos, args.ref_base, args.alt_base)], threads=1)
    print(lines[(ctg, pos)])


def tag_row(row, line):
    """update_filter_info (:486-518) for one evaluated call, `line` = its output line"""
    f = line.split()
    c = row.split("\t")
    if not str2bool(f[2]):
        c[5], c[6] = "0.0000", "LowQual"
    for ok, tag in zip(f[3:6] + f[7:8], ("ReadStartEnd", "VariantCluster", "StrandBias", "LowSeqEntropy")):
        if not str2bool(ok):
            c[6] += ";" + tag
    c[7] += ";SB={}".format(f[6])
    return "\t".join(c)


def postfilter(args):
    ctg_name, flanking = args.ctg_name, args.flanking
    if ctg_name is not None and "," in ctg_name and args.enable_postfilter:      # before anything is written
        sys.exit("[ERROR] clairs_to_amd postfilter_variants takes one contig in --ctg_name, or none (the reference's comma form is not implemented)")
    if not os.path.exists(args.output_dir):
        os.makedirs(args.output_dir, exist_ok=True)
    if not args.enable_postfilter:
        subprocess.run("ln -sf {} {}".format(args.pileup_vcf_fn, args.output_vcf_fn), shell=True)      # :597
        return
    header, pileup = read_vcf(args.pileup_vcf_fn, ctg_name, show_ref=args.show_ref, discard_indel=not args.is_indel,
                              filter_tag=args.input_filter_tag)
    out_header = header_up_to_last_format(header)
    vcf_folder = os.path.dirname(args.output_vcf_fn)
    if not os.path.exists(vcf_folder):
        print("[INFO] Output VCF folder {} not found, create it".format(vcf_folder))                    # shared/vcf.py:79-81
        if vcf_folder:
            os.makedirs(vcf_folder, exist_ok=True)
    fai = args.ref_fn + ".fai" if os.path.exists(args.ref_fn + ".fai") else ".".join(args.ref_fn.split(".")[:-1]) + ".fai"
    names = None if ctg_name is None else (ctg_name.split(",") if "," in ctg_name else [ctg_name])
    for row in open(fai):
        c = row.strip().split("\t")
        if names is None or c[0] in names:
            out_header += "##contig=<ID=%s,length=%s>\n" % (c[0], c[1])
    out_header += "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n"
    tuple_keys = ctg_name is None or "," in ctg_name
    with open(args.output_vcf_fn, "w") as out:
        out.write(out_header)
        calls = []
        with open(os.path.join(args.output_dir, "PF_INFO_INDEL" if args.is_indel else "PF_INFO_SNV"), "w") as f:
            for key, r in pileup.items():
                if r["filter"] != "PASS" or (args.test_pos and key != args.test_pos):
                    continue
                # :636-642
                ctg = ctg_name if ctg_name is not None else key[0]
                pos = key if ctg_name is not None else key[1]
                f.write(" ".join([ctg, str(pos), r["ref"], r["alt"], str(r["af"]), str(r["qual"])]) + "\n")
                calls.append((ctg, pos, r["ref"], r["alt"]))
        said = [0]

        def progress(n_done):                                   # :521-523, as the calls are evaluated
            while said[0] + 1000 <= n_done:
                said[0] += 1000
                print("[INFO] Postfilter variants: {} candidates processed".format(said[0]), flush=True)
        lines = evaluate_calls(args, calls, threads=max(1, int((args.threads or 4) * 4 / 5)), max_sites=args.job_max_sites,
                               max_span=args.job_max_span, progress=progress)
        for key in sorted(pileup):
            row = pileup[key]["row"].rstrip()
            k = key if tuple_keys else (ctg_name, key)
            out.write((tag_row(row, lines[k]) if k in lines else row) + "\n")
    return lines


def build_parser():
    p = ArgumentParser(description="Post-filtering for short-read data (window rules on the GPU)")
    p.add_argument("--tumor_bam_fn", type=str, default=None)
    p.add_argument("--ref_fn", type=str, default=None)
    p.add_argument("--ctg_name", type=str, default=None)
    p.add_argument("--pileup_vcf_fn", type=str, default=None)
    p.add_argument("--output_vcf_fn", type=str, default=None)
    p.add_argument("--output_dir", type=str, default=None)
    p.add_argument("--input_filter_tag", type=str_none, default=None)
    p.add_argument("--show_ref", action="store_true")
    p.add_argument("--samtools", type=str, default="samtools")
    p.add_argument("--mpileup_fn", type=str, default=None, help="prepared eight-column mpileup text instead of running samtools")
    p.add_argument("--enable_postfilter", type=str2bool, default=True)
    p.add_argument("--min_mq", type=int, default=20)             # shared/param.py:17
    p.add_argument("--min_bq", type=int, default=0)              # shared/param.py:19
    p.add_argument("--min_alt_coverage", type=int, default=2)
    p.add_argument("--is_indel", action="store_true")
    p.add_argument("--test_pos", type=int, default=None)
    p.add_argument("--flanking", type=int, default=100)
    p.add_argument("--disable_read_start_end_filtering", type=str2bool, default=False)
    p.add_argument("--job_max_sites", type=int, default=MAX_SITES_PER_JOB, help="calls per mpileup job (the result does not depend on it)")
    p.add_argument("--job_max_span", type=int, default=MAX_SPAN_PER_JOB, help="reference span per mpileup job")
    # the per-position form (:824-837, postfilter_per_pos): --af / --qual are declared there and read nowhere
    p.add_argument("--pos", type=int, default=None)
    p.add_argument("--ref_base", type=str, default=None)
    p.add_argument("--alt_base", type=str, default=None)
    p.add_argument("--af", type=float, default=None)
    p.add_argument("--qual", type=float, default=None)
    # src/postfilter_variants.py:771-822: the interpreters and the process / chunk layout of the reference's workers.  --threads, when
    # given, sizes the producer pool here (4/5 of it, as :585); the output does not depend on it.
    add_ignored(p, python="str", pypy3="str", parallel="str", threads="int", debug="flag", postfilter_variants_chunk_mode="bool",
                postfilter_chunk_max_sites="int", postfilter_chunk_max_span="int")
    return p


def main(argv=None):
    a = build_parser().parse_args(argv)
    if a.pos is None:
        postfilter(a)
    else:
        postfilter_per_pos(a)


if __name__ == "__main__":
    main()
