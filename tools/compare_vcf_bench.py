#!/usr/bin/env python3
"""Where compare_vcf's time goes, on seeded files of two sizes that bracket a real truth set:

    somatic   40,000 truth records,    60,000 calls   (a somatic truth set such as SEQC2's HCC1395: some 40 thousand SNVs)
    germline  4,000,000 truth records, 2,000,000 calls (a germline truth set of a whole genome: some four million records)

each with and without --output_best_f1_score and --roc_fn.  Timed per run: parsing (both VCFs and the BED, in Python), building the
record tables (Python), cto_compare_calls on the device (wall clock of the call, and its kernel_ms), the host path of the same call, the
whole command, and - when a reference checkout is given and the run is no larger than --reference_max_records - the reference's own
compare_vcf on the same files.  One JSON line per run is appended to --out (profiles/compare_vcf_bench.jsonl).  No test asserts a time.

    python tools/compare_vcf_bench.py [--sizes somatic,germline] [--reference DIR] [--out profiles/compare_vcf_bench.jsonl]"""
import argparse
import contextlib
import io
import json
import os
import random
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"somatic": (40000, 60000), "germline": (4000000, 2000000)}
CONTIGS = [("chr%d" % (i + 1), 240000000 - 8000000 * i) for i in range(22)]
REF_CHILD = r"""
import json, sys, time
sys.path.insert(0, sys.argv[1])
import src.compare_vcf as m
sys.argv = ["compare_vcf"] + json.loads(sys.argv[2])
t = time.perf_counter()
m.main()
sys.stderr.write("SECONDS %.6f\n" % (time.perf_counter() - t))
"""


def write_files(d, n_truth, n_calls, seed):
    """a truth VCF, a call VCF that shares about two thirds of its keys with it, and a BED of 20 kb in every 30 kb"""
    rng = random.Random(seed)
    head = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n"
    total = sum(n for _, n in CONTIGS)
    keys = []
    for ctg, length in CONTIGS:
        for p in sorted(rng.sample(range(1, length), max(1, n_truth * length // total))):
            keys.append((ctg, p, rng.choice("CGT")))
    with open(os.path.join(d, "truth.vcf"), "w") as f:
        f.write(head)
        for ctg, p, alt in keys:
            f.write("%s\t%d\t.\tA\t%s\t.\tPASS\t.\tGT\t0/1\n" % (ctg, p, alt))
    with open(os.path.join(d, "calls.vcf"), "w") as f:
        f.write(head)
        step = max(1, len(keys) * 3 // (2 * n_calls))
        written = 0
        for ctg, p, alt in keys[::step]:
            if written >= n_calls:
                break
            f.write("%s\t%d\t.\tA\t%s\t%.2f\tPASS\t.\tGT:GQ:DP:AF\t0/1:10:30:0.4\n" % (ctg, p, alt if rng.random() < 0.9 else "A", rng.random() * 60))
            written += 1
            if written < n_calls and rng.random() < 0.5:
                f.write("%s\t%d\t.\tA\tC\t%.2f\tPASS\t.\tGT:GQ:DP:AF\t0/1:10:30:0.1\n" % (ctg, p + 1, rng.random() * 30))
                written += 1
    with open(os.path.join(d, "conf.bed"), "w") as f:
        for ctg, length in CONTIGS:
            for s in range(0, length, 30000):
                f.write("%s\t%d\t%d\n" % (ctg, s, min(length, s + 20000)))
    return written


def one_run(d, size, sweeps, reference, reference_max):
    import numpy as np
    from collections import OrderedDict
    from clairs_to_amd import compare_vcf as cv
    from clairs_to_amd.cal_af_distribution import read_vcf
    import torch
    argv = ["--truth_vcf_fn", os.path.join(d, "truth.vcf"), "--input_vcf_fn", os.path.join(d, "calls.vcf"), "--bed_fn", os.path.join(d, "conf.bed"),
            "--input_filter_tag", "PASS"]
    if sweeps:
        argv += ["--output_best_f1_score", "--roc_fn", os.path.join(d, "roc.txt")]
    row = dict(size=size, sweeps=sweeps, device=torch.cuda.get_device_name(0) if torch.cuda.is_available() else None)
    t0 = time.perf_counter()
    truth = read_vcf(argv[1], None, None, skip_genotype=True)
    calls = read_vcf(argv[3], None, "PASS", skip_genotype=True, keep_af=True, discard_indel=True)
    bed = cv.bed_tree_from(argv[5])
    t1 = time.perf_counter()
    contigs, alleles = OrderedDict(), {}
    tin, ttr = cv._table(calls, contigs, alleles, None, set(), False), cv._table(truth, contigs, alleles, None, set(), False)
    for name in bed.intervals:
        contigs.setdefault(name, len(contigs))
    beds = cv.pack_beds([bed], contigs)
    finite = tin["qual"][np.isfinite(tin["qual"])]
    cut, roc = (np.unique(np.trunc(finite)), np.unique(finite)) if sweeps else ((), ())
    t2 = time.perf_counter()
    row.update(n_truth=len(truth), n_calls=len(calls), n_intervals=int(len(beds[2])), n_cutoffs=int(len(cut) + len(roc)), parse_s=t1 - t0, tables_s=t2 - t1)
    results = {}
    for where in (("device", "host") if row["device"] else ("host",)):
        best, stats = None, {}
        for _ in range(3):                                         # the first call grows the buffers and loads the code object
            t = time.perf_counter()
            results[where] = cv.compare_calls(tin, ttr, beds, len(contigs), cutoffs=cut, roc_cutoffs=roc, where=where, stats=stats)
            best = min(best or 1e30, time.perf_counter() - t)
        row["call_%s_s" % where] = best
        if where == "device":
            row["kernel_ms"] = stats["kernel_ms"]
    if len(results) == 2:
        assert all(np.array_equal(results["device"][k], results["host"][k]) for k in ("input_sets", "truth_sets", "sweep", "roc_sweep"))
        assert results["device"]["counters"] == results["host"]["counters"]
    row["counters"] = results["host"]["counters"]
    t = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        cv.main(argv)
    row["command_s"] = time.perf_counter() - t
    host_side = row["parse_s"] + row["tables_s"]
    row["python_share"] = host_side / (host_side + row["call_device_s" if row["device"] else "call_host_s"])    # parsing and tables, of the three stages
    row["reference_s"] = None
    if reference and os.path.isdir(reference) and row["n_truth"] + row["n_calls"] <= reference_max:
        p = subprocess.run([sys.executable, "-W", "ignore", "-c", REF_CHILD, reference, json.dumps(argv)], cwd=d, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                           text=True)
        if p.returncode == 0:
            row["reference_s"] = float([ln for ln in p.stderr.split("\n") if ln.startswith("SECONDS ")][-1].split()[1])
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="somatic,germline")
    ap.add_argument("--reference", default=None, help="a checkout of the reference: its compare_vcf is timed on the same files")
    ap.add_argument("--reference_max_records", type=int, default=200000, help="the reference's sweeps are quadratic under CPython")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compare_vcf_bench.jsonl"))
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for size in args.sizes.split(","):
        with tempfile.TemporaryDirectory(prefix="compare_vcf_bench_") as d:
            write_files(d, SIZES[size][0], SIZES[size][1], args.seed)
            for sweeps in (False, True):
                row = one_run(d, size, sweeps, args.reference, args.reference_max_records)
                print(json.dumps(row), flush=True)
                with open(args.out, "a") as f:
                    f.write(json.dumps(row, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
