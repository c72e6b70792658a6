"""Time of the purity/ploidy grid of run_ascat on the default grid (100 ploidies x 95 purities): the reference's create_distance_matrix
from a checkout (--ref-src; skipped when it is not given, does not exist or cannot be imported), the host path of cto_ascat_distance
(threads over cells) and the kernel.  Each leg: --warmup calls, then --repeats timed calls, reported as median [min-max]; one JSON line
per leg and segment count is appended to profiles/ascat_bench.jsonl.  The host and device legs must return the same bits.
    python tools/ascat_bench.py [--segments 200 2000] [--legs reference host device] [--ref-src DIR] [--out FILE]
The job: --segments segments with a logR around 0 (sd 0.4), a BAF in 0.02 .. 0.5 (a fifth at exactly 0.5) and 1 - 59 probes, numpy seed 1,
gamma 1.  The host and device legs time the C call, the per-segment terms (the power) included; the reference leg is numpy called from
CPython, one cell at a time, and is timed on --ref-repeats calls after one warm-up."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_job(n, seed=1):
    rng = np.random.default_rng(seed)
    s = np.column_stack((rng.normal(0, 0.4, size=n), rng.uniform(0.02, 0.5, size=n), rng.integers(1, 60, size=n).astype(float)))
    s[rng.random(n) < 0.2, 1] = 0.5
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, nargs="+", default=[200, 2000])
    ap.add_argument("--legs", nargs="+", default=["reference", "host", "device"], choices=["reference", "host", "device"])
    ap.add_argument("--ref-src", default=None, help="checkout of the reference (its src/verdict/run_ascat.py is imported)")
    ap.add_argument("--ref-repeats", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ascat_bench.jsonl"))
    a = ap.parse_args()
    for n in a.segments:
        s = make_job(n)
        job = "default grid 100 x 95, %d segments, gamma 1, numpy seed 1" % n
        print("job:", job)
        results = {}
        for leg in a.legs:
            stats = {}
            warmup, repeats = a.warmup, a.repeats
            if leg == "reference":
                src = os.path.join(a.ref_src, "src", "verdict") if a.ref_src else None
                if not src or not os.path.isdir(src):
                    print("ascat_bench: no reference checkout (--ref-src), the reference leg is skipped")
                    continue
                sys.path.insert(0, src)
                try:
                    import run_ascat as ref
                except ImportError as e:
                    print("ascat_bench: the reference's module does not import (%s), the reference leg is skipped" % e)
                    continue
                warmup, repeats = 1, a.ref_repeats

                def call():
                    results["reference"] = ref.create_distance_matrix(s, 1.0, min_ploidy=1.5, max_ploidy=5.5, min_purity=0.1, max_purity=1.05)
            else:
                if leg == "device":
                    import torch
                    if not torch.cuda.is_available():
                        sys.exit("ascat_bench: no GPU for the device leg")
                from clairs_to_amd.run_ascat import create_distance_matrix

                def call(leg=leg, stats=stats):
                    results[leg] = create_distance_matrix(s, 1.0, 1.5, 5.5, 0.1, 1.05, leg, stats)
            walls, kernel_ms = [], []
            for it in range(warmup + repeats):
                t0 = time.perf_counter()
                call()
                if it >= warmup:
                    walls.append(time.perf_counter() - t0)
                    kernel_ms.append(stats.get("kernel_ms", 0.0))
            w = np.array(walls) * 1e3
            rec = dict(tool="ascat_bench", leg=leg, job=job, cells=int(results[leg].size), segments=n, host_path=stats.get("host_path"), warmup=warmup,
                       repeats=repeats, call_ms_median=round(float(np.median(w)), 3), call_ms_min=round(float(w.min()), 3),
                       call_ms_max=round(float(w.max()), 3), kernel_ms_median=round(float(np.median(kernel_ms)), 4) if leg == "device" else None,
                       cpus=len(os.sched_getaffinity(0)), interpreter="CPython %s" % sys.version.split()[0], numpy=np.__version__)
            print(json.dumps(rec))
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")
        bits = {leg: d.view(np.uint64) for leg, d in results.items()}
        if "host" in bits and "device" in bits:
            if not (bits["host"] == bits["device"]).all():
                sys.exit("ascat_bench: the host and device legs differ")
            print("host and device: the same bits")
        if "reference" in bits and "host" in bits:
            if not (bits["reference"] == bits["host"]).all():
                sys.exit("ascat_bench: the reference and host legs differ")
            print("reference and host: the same bits")
    return 0


if __name__ == "__main__":
    main()
