"""Time of correct_logr at two row counts: the reference's correctLogR from a checkout (--ref-src; skipped when it is not given, does not
exist or cannot be imported - it needs scipy and scikit-learn), the host path of cto_correct_logr and the kernels.  Our legs split the
step in two: reading the three text tables into arrays (Python, the same for both legs) and the C call; the reference leg is its whole
function, files to file.  Each of our legs: --warmup calls, then --repeats timed calls, reported as median [min-max]; the reference leg
is timed once after no warm-up.  One JSON line per leg and row count is appended to profiles/correct_logr_bench.jsonl.  The host and
device legs must return the same bits: the tool exits non-zero otherwise.
    python tools/correct_logr_bench.py [--rows 20000 200000] [--legs reference host device] [--ref-src DIR] [--out FILE]
The job: --rows probes on one chromosome, 18 GC columns and 12 replication-timing columns carrying two latent tracks, six decimals in the
files, numpy seed 1."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
G, T = 18, 12


def write_job(d, n, seed=1):
    rng = np.random.default_rng(seed)
    a, b = rng.beta(4, 6, size=n), rng.normal(0, 1, size=n)
    gc = np.clip(rng.uniform(0.2, 0.9, size=(1, G)) * a[:, None] + rng.uniform(0, 0.3, size=(n, G)), 0, 1)
    rt = 40 + rng.uniform(5, 20, size=(1, T)) * b[:, None] + rng.normal(0, 6, size=(n, T))
    logr = -1.8 * (a - 0.4) + 6 * (a - 0.4) ** 2 + 0.06 * b + rng.normal(0, 0.12, size=n)
    pos = np.cumsum(rng.integers(50, 5000, size=n))
    with open(os.path.join(d, "logr.txt"), "w") as f:
        f.write("Chromosome\tPosition\tS\n")
        f.writelines("chr1\t%d\t%r\n" % (p, float(v)) for p, v in zip(pos, logr))
    for name, table in (("gc.txt", gc), ("rt.txt", rt)):
        with open(os.path.join(d, name), "w") as f:
            f.write("\tChr\tPosition\t" + "\t".join("c%d" % j for j in range(table.shape[1])) + "\n")
            f.writelines("snp%d\t1\t%d\t%s\n" % (i, p, "\t".join("%.6f" % v for v in row)) for i, (p, row) in enumerate(zip(pos, table)))


def spread(seconds):
    w = np.array(seconds) * 1e3
    return dict(median=round(float(np.median(w)), 3), min=round(float(w.min()), 3), max=round(float(w.max()), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[20000, 200000])
    ap.add_argument("--legs", nargs="+", default=["reference", "host", "device"], choices=["reference", "host", "device"])
    ap.add_argument("--ref-src", default=None, help="checkout of the reference (its src/verdict/correct_logr.py is imported)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "correct_logr_bench.jsonl"))
    a = ap.parse_args()
    from clairs_to_amd.correct_logr import fit, read_annotation, rows_of
    from clairs_to_amd.predict_germline_genotypes import read_table
    for n in a.rows:
        d = tempfile.mkdtemp(prefix="correct_logr_bench_")
        write_job(d, n)
        paths = [os.path.join(d, k) for k in ("logr.txt", "gc.txt", "rt.txt")]
        job = "%d probes, %d GC and %d replication-timing columns, numpy seed 1" % (n, G, T)
        print("job:", job)
        common = dict(tool="correct_logr_bench", job=job, rows=n, cpus=len(os.sched_getaffinity(0)), interpreter="CPython %s" % sys.version.split()[0],
                      numpy=np.__version__)
        results, parse_s = {}, []
        for _ in range(2):
            t0 = time.perf_counter()
            logr_table = read_table(paths[0])
            keys = list(logr_table)
            logr = np.array(list(logr_table.values())).astype(float)
            gc, rt = rows_of(read_annotation(paths[1]), keys, "GC content"), rows_of(read_annotation(paths[2]), keys, "replication timing")
            parse_s.append(time.perf_counter() - t0)
        recs = []
        for leg in a.legs:
            if leg == "reference":
                src = os.path.join(a.ref_src, "src", "verdict") if a.ref_src else None
                if not src or not os.path.isdir(src):
                    print("correct_logr_bench: no reference checkout (--ref-src), the reference leg is skipped")
                    continue
                sys.path.insert(0, src)
                try:
                    import correct_logr as ref
                except ImportError as e:
                    print("correct_logr_bench: the reference's module does not import (%s), the reference leg is skipped" % e)
                    continue
                t0 = time.perf_counter()
                ref.correctLogR(*paths, os.path.join(d, "ref_out.txt"), "S")
                recs.append(dict(common, leg=leg, whole_ms=round((time.perf_counter() - t0) * 1e3, 1), repeats=1))
                continue
            if leg == "device":
                import torch
                if not torch.cuda.is_available():
                    sys.exit("correct_logr_bench: no GPU for the device leg")
            walls, kernel_ms, stats = [], [], {}
            for it in range(a.warmup + a.repeats):
                t0 = time.perf_counter()
                results[leg] = fit(logr, gc, rt, leg, stats)
                if it >= a.warmup:
                    walls.append(time.perf_counter() - t0)
                    kernel_ms.append(stats["kernel_ms"])
            recs.append(dict(common, leg=leg, host_path=stats["host_path"], columns=[stats["col_insert"], stats["col_amplic"], stats["col_replic"]],
                             warmup=a.warmup, repeats=a.repeats, parse_ms=spread(parse_s), call_ms=spread(walls),
                             kernel_ms_median=round(float(np.median(kernel_ms)), 4) if leg == "device" else None,
                             input_mb=round((logr.nbytes + gc.nbytes + rt.nbytes) / 1e6, 2)))
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            for rec in recs:
                print(json.dumps(rec))
                f.write(json.dumps(rec) + "\n")
        if "host" in results and "device" in results:
            for h, v in zip(results["host"], results["device"]):
                if not (h.view(np.uint64) == v.view(np.uint64)).all():
                    sys.exit("correct_logr_bench: the host and device legs differ")
            print("host and device: the same bits")
    return 0


if __name__ == "__main__":
    main()
