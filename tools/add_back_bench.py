#!/usr/bin/env python3
"""Where add_back_missing_variants_in_genotyping's time goes, on seeded files of two sizes:

    panel   20,000 list sites     (a targeted panel or an exome's known sites)
    genome  2,000,000 list sites  (a COSMIC- or dbSNP-sized list)

each with calls for 2 % of the sites and a _hybrid_info row for every site.  Timed per size: reading the files, cto_add_back on the device
(wall clock of the call, best of three, and its kernel_ms), the host path of the same call on 16 threads, the whole command (files in,
file out), the module's Python restatement and - when a reference checkout is given and the size is no larger than --reference_max_sites -
the reference's own command on the same files.  Device and host bytes are compared.  One JSON line per size is appended to --out
(profiles/add_back_bench.jsonl).  No test asserts a time.

    python tools/add_back_bench.py [--sizes panel,genome] [--where device,host] [--reference DIR] [--out profiles/add_back_bench.jsonl]"""
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

SIZES = {"panel": 20000, "genome": 2000000}
CONTIGS = [("chr%d" % (i + 1), 240000000 - 8000000 * i) for i in range(22)]
REF_CHILD = r"""
import json, sys, time
sys.path.insert(0, sys.argv[1])
import src.add_back_missing_variants_in_genotyping as m
sys.argv = ["add_back"] + json.loads(sys.argv[2])
t = time.perf_counter()
m.main()
sys.stderr.write("SECONDS %.6f\n" % (time.perf_counter() - t))
"""


def write_files(d, n_sites, seed):
    rng = random.Random(seed)
    head = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n"
    total = sum(n for _, n in CONTIGS)
    os.makedirs(os.path.join(d, "cand"))
    with open(os.path.join(d, "list.vcf"), "w") as fl, open(os.path.join(d, "calls.vcf"), "w") as fc:
        fl.write(head)
        fc.write(head)
        for ctg, length in CONTIGS:
            with open(os.path.join(d, "cand", "%s.0_hybrid_info" % ctg), "w") as fi:
                for p in sorted(rng.sample(range(1, length), max(1, n_sites * length // total))):
                    ref, alt = rng.choice("ACGT"), rng.choice("ACGT")
                    fl.write("%s\t%d\trs%d\t%s\t%s\t.\tPASS\tAC=3;AN=200\n" % (ctg, p, p, ref, alt))
                    if rng.random() < 0.02:
                        fc.write("%s\t%d\t.\t%s\t%s\t%.4f\tPASS\tH\tGT:GQ:DP:AF\t0/1:12:40:0.2500\n" % (ctg, p, ref, alt, rng.random() * 30))
                    dp = rng.randrange(10, 90)
                    fi.write("%s\t%d\t%s\t%d-%s %d %s %d\n" % (ctg, p, ref, dp, ref, dp - 2, alt, 2))


def one_run(d, size, wheres, reference, reference_max):
    import torch
    from clairs_to_amd import add_back_missing_variants_in_genotyping as m
    argv = ["--genotyping_mode_vcf_fn", os.path.join(d, "list.vcf"), "--call_fn", os.path.join(d, "calls.vcf"), "--candidates_folder", os.path.join(d, "cand"),
            "--output_fn", os.path.join(d, "out.vcf")]
    row = dict(size=size, n_sites=SIZES[size], device=torch.cuda.get_device_name(0) if torch.cuda.is_available() else None)
    t = time.perf_counter()
    calls, listed, info = m.read_text(argv[3]), m.read_text(argv[1]), m.read_info_folder(argv[5])
    row.update(read_s=time.perf_counter() - t, bytes_in=len(calls) + len(listed) + len(info))
    results = {}
    for where in wheres:
        best, stats = None, {}
        for _ in range(3):                                         # the first call grows the buffers and loads the code object
            t = time.perf_counter()
            results[where] = m.add_back(calls, listed, info, m.GENOTYPING, True, where=where, host_threads=16, stats=stats)
            best = min(best or 1e30, time.perf_counter() - t)
        assert stats["restated"] is None
        row["call_%s_s" % where] = best
        if where == "device":
            row["kernel_ms"] = stats["kernel_ms"]
    if len(results) == 2:
        assert results["device"] == results["host"]
    any_result = next(iter(results.values()))
    row.update(bytes_out=len(any_result[0]), counts=list(any_result[1]))
    t = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        m.main(argv + ["--where", wheres[0]])
    row["command_s"] = time.perf_counter() - t
    row["command_where"] = wheres[0]
    t = time.perf_counter()
    restated = m.restate(calls, listed, info, m.GENOTYPING, True)
    row["restatement_s"] = time.perf_counter() - t
    assert restated == any_result
    row["reference_s"] = None
    if reference and os.path.isdir(reference) and SIZES[size] <= reference_max:
        p = subprocess.run([sys.executable, "-W", "ignore", "-c", REF_CHILD, reference, json.dumps(argv)], cwd=d, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                           text=True)
        if p.returncode == 0:
            row["reference_s"] = float([ln for ln in p.stderr.split("\n") if ln.startswith("SECONDS ")][-1].split()[1])
            assert open(argv[7], "rb").read() == any_result[0]
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="panel,genome")
    ap.add_argument("--where", default=None, help="device,host (default: both with a GPU, host without)")
    ap.add_argument("--reference", default=None, help="a checkout of the reference: its command is timed on the same files")
    ap.add_argument("--reference_max_sites", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "add_back_bench.jsonl"))
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    import torch
    wheres = args.where.split(",") if args.where else (["device", "host"] if torch.cuda.is_available() else ["host"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for size in args.sizes.split(","):
        with tempfile.TemporaryDirectory(prefix="add_back_bench_") as d:
            write_files(d, SIZES[size], args.seed)
            row = one_run(d, size, wheres, args.reference, args.reference_max_sites)
            print(json.dumps(row), flush=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(row, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
