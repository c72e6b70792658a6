"""Time of the hot path of tag_germline_variant - per call the scan of the segment table and the binomial tests - on 2 000 calls against
200 segments and 20 000 calls against 2 000: the reference's tag_germline_variant from a checkout (--ref-src; skipped when it is not
given, does not exist or cannot be imported - it needs scipy), the host path of cto_tag_germline (threads over calls) and the kernel.
Each leg: --warmup calls, then --repeats timed calls, reported as median [min-max]; one JSON line per leg and job is appended to
profiles/tag_germline_bench.jsonl.  The host and device legs must return the same bits.
    python tools/tag_germline_bench.py [--calls 2000 20000] [--segments 200 2000] [--legs reference host device] [--ref-src DIR] [--out FILE]
The job: segments of 100 kb, end to end, on four contigs, nMajor 0 - 4 and nMinor 0 - 2, written in a shuffled order; calls anywhere on the
contigs' covered part, a depth of 30 - 300, an AF with four decimals, purity 0.4, numpy seed 1.  The host and device legs time the C call
alone.  The reference leg times its whole function on the same calls as a VCF, file reading and writing included (they are a small part:
it spends its time in scipy.stats.binomtest and in the scan), once after no warm-up, with the three builtins its `from numpy import *`
hides put back into its namespace (under numpy 2 it does not run otherwise)."""
import argparse
import builtins
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONTIGS = 4


def make_job(n_calls, n_segments, seed=1):
    rng = np.random.default_rng(seed)
    per = -(-n_segments // CONTIGS)
    order = rng.permutation(n_segments)
    table = dict(seg_chr=(order // per).astype(np.int32), seg_start=(order % per) * 100000 + 1, seg_end=(order % per + 1) * 100000,
                 seg_nmaj=rng.integers(0, 5, size=n_segments), seg_nmin=rng.integers(0, 3, size=n_segments))
    calls = dict(ctg=rng.integers(0, CONTIGS, size=n_calls).astype(np.int32), pos=rng.integers(1, per * 100000 + 1, size=n_calls),
                 depth=rng.integers(30, 301, size=n_calls), freq=np.round(rng.random(n_calls), 4))
    return calls, table


def write_files(d, calls, table):
    with open(os.path.join(d, "in.vcf"), "w") as f:
        f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n")
        for c, p, n, a in zip(calls["ctg"], calls["pos"], calls["depth"], calls["freq"]):
            f.write("chr%d\t%d\t.\tA\tG\t20.0\tPASS\t.\tGT:GQ:DP:AF\t0/1:20:%d:%.4f\n" % (c + 1, p, n, a))
    with open(os.path.join(d, "cna.txt"), "w") as f:
        f.write("Sample\tChromosome\tStartPosition\tEndPosition\tnMajor\tnMinor\n")
        for row in zip(table["seg_chr"], table["seg_start"], table["seg_end"], table["seg_nmaj"], table["seg_nmin"]):
            f.write("T\tchr%d\t%d\t%d\t%d\t%d\n" % ((row[0] + 1,) + row[1:]))
    with open(os.path.join(d, "purity.txt"), "w") as f:
        f.write("Sample\tPurity\tPloidy\tGoodnessOfFit\nT\t0.4\t2.0\t99.0\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, nargs="+", default=[2000, 20000])
    ap.add_argument("--segments", type=int, nargs="+", default=[200, 2000])
    ap.add_argument("--legs", nargs="+", default=["reference", "host", "device"], choices=["reference", "host", "device"])
    ap.add_argument("--ref-src", default=None, help="checkout of the reference (its src/verdict/tag_germline_variant.py is imported)")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--machine", default=None, help="a label for the machine, written into every line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tag_germline_bench.jsonl"))
    a = ap.parse_args()
    if len(a.calls) != len(a.segments):
        sys.exit("tag_germline_bench: --calls and --segments go in pairs")
    for n_calls, n_segments in zip(a.calls, a.segments):
        calls, table = make_job(n_calls, n_segments)
        job = "%d calls of depth 30-300 against %d segments, purity 0.4, numpy seed 1" % (n_calls, n_segments)
        print("job:", job)
        results = {}
        for leg in a.legs:
            stats = {}
            warmup, repeats = a.warmup, a.repeats
            if leg == "reference":
                src = os.path.join(a.ref_src, "src", "verdict") if a.ref_src else None
                if not src or not os.path.isdir(src):
                    print("tag_germline_bench: no reference checkout (--ref-src), the reference leg is skipped")
                    continue
                sys.path.insert(0, src)
                try:
                    import tag_germline_variant as ref
                except ImportError as e:
                    print("tag_germline_bench: the reference's module does not import (%s), the reference leg is skipped" % e)
                    continue
                ref.round, ref.max, ref.min = builtins.round, builtins.max, builtins.min
                warmup, repeats = 0, 1
                d = tempfile.mkdtemp(prefix="tag_germline_bench_")
                write_files(d, calls, table)
                ns = argparse.Namespace(input_vcf_fn=os.path.join(d, "in.vcf"), output_fn=os.path.join(d, "out.vcf"),
                                        tumor_purity_ploidy_output_file=os.path.join(d, "purity.txt"), tumor_cna_output_file=os.path.join(d, "cna.txt"))

                def call(ns=ns):
                    ref.tag_germline_variant(ns)
                    results["reference"] = None
            else:
                if leg == "device":
                    import torch
                    if not torch.cuda.is_available():
                        sys.exit("tag_germline_bench: no GPU for the device leg")
                from clairs_to_amd.tag_germline_variant import tag_calls

                def call(leg=leg, stats=stats):
                    results[leg] = tag_calls(calls["ctg"], calls["pos"], calls["depth"], calls["freq"], table["seg_chr"], table["seg_start"], table["seg_end"],
                                             table["seg_nmaj"], table["seg_nmin"], 0.4, leg, stats)
            walls, kernel_ms = [], []
            for it in range(warmup + repeats):
                t0 = time.perf_counter()
                call()
                if it >= warmup:
                    walls.append(time.perf_counter() - t0)
                    kernel_ms.append(stats.get("kernel_ms", 0.0))
            w = np.array(walls) * 1e3
            rec = dict(tool="tag_germline_bench", leg=leg, job=job, calls=n_calls, segments=n_segments, calls_with_segment=stats.get("n_with_segment"),
                       tests=stats.get("n_tests"), host_path=stats.get("host_path"), warmup=warmup, repeats=repeats, call_ms_median=round(float(np.median(w)), 3),
                       call_ms_min=round(float(w.min()), 3), call_ms_max=round(float(w.max()), 3),
                       kernel_ms_median=round(float(np.median(kernel_ms)), 4) if leg == "device" else None, machine=a.machine,
                       cpus=len(os.sched_getaffinity(0)), interpreter="CPython %s" % sys.version.split()[0], numpy=np.__version__)
            print(json.dumps(rec))
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")
        if results.get("host") is not None and results.get("device") is not None:
            for h, d in zip(results["host"], results["device"]):
                if not (h.view(np.uint8) == d.view(np.uint8)).all():
                    sys.exit("tag_germline_bench: the host and device legs differ")
            print("host and device: the same bits")
    return 0


if __name__ == "__main__":
    main()
