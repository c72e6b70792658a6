"""Wall time of predict_germline_genotypes (tumour-only branch) on one synthetic BAF table: the reference's predictGermlineGenotypes from a
checkout (--ref-src; skipped when it is not given or does not exist), our module through the host path of cto_germline_window_dist, and our
module through the kernel.  Each leg: --warmup calls, then --repeats timed calls, reported as median [min-max]; one JSON line per leg is
appended to profiles/germline_bench.jsonl.  The three legs must write the same file.
    python tools/germline_bench.py [--rows 60000] [--legs reference host device] [--ref-src DIR] [--out FILE]
The table: --rows loci over chr1..chr22, chrX in proportion to their lengths, every third locus heterozygous (BAF = alt / depth, alt
binomial around half of a depth of 200 - 400), the others homozygous (at most 2 reads of the other allele), numpy seed 1.  The reference
leg is CPython over every undecided probe: about 0.6 ms per probe, so --rows is small next to a whole-genome 1000G set (several million)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHR_MB = [248, 242, 198, 190, 181, 171, 159, 145, 138, 133, 135, 133, 114, 107, 102, 90, 83, 80, 58, 64, 46, 50, 156]


def write_table(d, rows, seed=1):
    rng = np.random.default_rng(seed)
    per_chr = np.maximum(1, np.round(np.array(CHR_MB) / sum(CHR_MB) * rows).astype(int))
    baf_fn, logr_fn = os.path.join(d, "Tumor_BAF.txt"), os.path.join(d, "Tumor_LogR.txt")
    with open(baf_fn, "w") as fb, open(logr_fn, "w") as fl:
        fb.write("Chromosome\tPosition\tS\n")
        fl.write("Chromosome\tPosition\tS\n")
        i = 0
        for ci, n in enumerate(per_chr):
            name = "chr%s" % (ci + 1 if ci < 22 else "X")
            pos = np.sort(rng.choice(CHR_MB[ci] * 1000000, size=n, replace=False)) + 1
            depth = rng.integers(200, 401, size=n)
            het = (np.arange(i, i + n) % 3) == 0
            alt = np.where(het, rng.binomial(depth, 0.5), np.where(rng.random(n) < 0.5, rng.integers(0, 3, size=n), depth - rng.integers(0, 3, size=n)))
            for p, a, dp in zip(pos.tolist(), alt.tolist(), depth.tolist()):
                fb.write("%s\t%d\t%s\n" % (name, p, str(a / dp)))
                fl.write("%s\t%d\t0.0\n" % (name, p))
            i += n
    return baf_fn, logr_fn, int(per_chr.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=60000)
    ap.add_argument("--legs", nargs="+", default=["reference", "host", "device"], choices=["reference", "host", "device"])
    ap.add_argument("--ref-src", default=None, help="checkout of the reference (its src/verdict/predict_germline_genotypes.py is imported)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "germline_bench.jsonl"))
    a = ap.parse_args()
    d = tempfile.mkdtemp(prefix="germline_bench_")
    baf_fn, logr_fn, rows = write_table(d, a.rows)
    table = "%d loci over chr1..22, X by length, every third heterozygous (alt ~ Binomial(depth, 0.5), depth 200-400), numpy seed 1" % rows
    print("table:", table)
    outputs = {}
    for leg in a.legs:
        out_fn = os.path.join(d, "GG_%s.txt" % leg)
        stats = {}
        if leg == "reference":
            src = os.path.join(a.ref_src, "src", "verdict") if a.ref_src else None
            if not src or not os.path.isdir(src):
                print("germline_bench: no reference checkout (--ref-src), the reference leg is skipped")
                continue
            sys.path.insert(0, src)
            from predict_germline_genotypes import predictGermlineGenotypes
            call = lambda: predictGermlineGenotypes(logr_fn, baf_fn, None, out_fn, 0.02, 0.30, 0.65, 0.03, 100, "S")
        else:
            if leg == "device":
                import torch
                if not torch.cuda.is_available():
                    sys.exit("germline_bench: no GPU for the device leg")
            from clairs_to_amd.predict_germline_genotypes import predict_germline_genotypes
            call = lambda: predict_germline_genotypes(logr_fn, baf_fn, None, out_fn, sample_name="S", where=leg, stats=stats)
        walls, kernel_ms = [], []
        for it in range(a.warmup + a.repeats):
            t0 = time.perf_counter()
            call()
            if it >= a.warmup:
                walls.append(time.perf_counter() - t0)
                kernel_ms.append(stats.get("kernel_ms", 0.0))
        w = np.array(walls)
        outputs[leg] = open(out_fn).read()
        rec = dict(tool="germline_bench", leg=leg, table=table, rows=rows, undecided=stats.get("n_probes"), runs=stats.get("n_runs"),
                   host_path=stats.get("host_path"), heterozygous=outputs[leg].count("\tFalse\n"), warmup=a.warmup, repeats=a.repeats,
                   wall_s_median=round(float(np.median(w)), 5), wall_s_min=round(float(w.min()), 5), wall_s_max=round(float(w.max()), 5),
                   kernel_ms_median=round(float(np.median(kernel_ms)), 4) if leg == "device" else None,
                   cpus=len(os.sched_getaffinity(0)), interpreter="CPython %s" % sys.version.split()[0])
        print(json.dumps(rec))
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
    if len(set(outputs.values())) > 1:
        sys.exit("germline_bench: the legs wrote different files: %s" % sorted(outputs))


if __name__ == "__main__":
    main()
