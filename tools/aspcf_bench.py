"""Time of the window fits of aspcf on one genome-shaped job: the reference's aspcfpart from a checkout (--ref-src; skipped when it is not
given, does not exist or cannot be imported - it needs scipy), the host path of cto_aspcf_windows (threads over windows) and the kernel.
Each leg: --warmup calls, then --repeats timed calls, reported as median [min-max]; one JSON line per leg is appended to
profiles/aspcf_bench.jsonl.  The host and device legs must return the same bits.
    python tools/aspcf_bench.py [--windows 1500] [--gamma 1000] [--legs reference host device] [--ref-src DIR] [--ref-windows 8] [--out FILE]
The job: --windows windows of 1000 heterozygous probes, each starting 800 after the one before (the reference's schedule on one long
chromosome), over tracks with a level change every 5 - 60 probes (logR: levels in -0.8 .. 0.8, noise 0.1; flipped BAF: 0.2 .. 0.5, noise
0.03), divisors as a MAD squared would be, numpy seed 1.  The reference leg is numpy called from CPython, one window at a time: it runs the
first --ref-windows windows only and reports the time per window."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_job(n_win, seed=1):
    rng = np.random.default_rng(seed)
    n = 800 * (n_win - 1) + 1000
    y1, y2 = np.empty(n), np.empty(n)
    i = 0
    while i < n:
        m = int(rng.integers(5, 61))
        y1[i:i + m] = rng.uniform(-0.8, 0.8) + rng.normal(0, 0.1, size=len(y1[i:i + m]))
        y2[i:i + m] = np.clip(0.5 - rng.uniform(0, 0.3) + rng.normal(0, 0.03, size=len(y2[i:i + m])), 0.01, 0.5)
        i += m
    lo = 800 * np.arange(n_win, dtype=np.int64)
    return y1, y2, lo, lo + 1000, rng.uniform(0.05, 0.2, size=n_win) ** 2, rng.uniform(0.01, 0.05, size=n_win) ** 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=1500)
    ap.add_argument("--gamma", type=float, default=1000)
    ap.add_argument("--legs", nargs="+", default=["reference", "host", "device"], choices=["reference", "host", "device"])
    ap.add_argument("--ref-src", default=None, help="checkout of the reference (its src/verdict/aspcf.py is imported)")
    ap.add_argument("--ref-windows", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aspcf_bench.jsonl"))
    a = ap.parse_args()
    y1, y2, lo, hi, v1, v2 = make_job(a.windows)
    job = "%d windows of 1000 probes, 800 apart, level changes every 5-60 probes, gamma %g, kmin 6, numpy seed 1" % (a.windows, a.gamma)
    print("job:", job)
    results = {}
    for leg in a.legs:
        stats = {}
        if leg == "reference":
            src = os.path.join(a.ref_src, "src", "verdict") if a.ref_src else None
            if not src or not os.path.isdir(src):
                print("aspcf_bench: no reference checkout (--ref-src), the reference leg is skipped")
                continue
            sys.path.insert(0, src)
            try:
                from aspcf import aspcfpart
            except ImportError as e:
                print("aspcf_bench: the reference's module does not import (%s), the reference leg is skipped" % e)
                continue
            n_ref = min(a.ref_windows, a.windows)

            def call():
                for k in range(n_ref):
                    aspcfpart(logRpart=y1[lo[k]:hi[k]], allBflip=y2[lo[k]:hi[k]], a=int(lo[k]), b=int(hi[k]), d=100, sd1=np.sqrt(v1[k]),
                              sd2=np.sqrt(v2[k]), N=len(y1), kmin=6, gamma=a.gamma)
        else:
            if leg == "device":
                import torch
                if not torch.cuda.is_available():
                    sys.exit("aspcf_bench: no GPU for the device leg")
            from clairs_to_amd.aspcf import aspcf_windows

            def call(leg=leg, stats=stats):
                results[leg] = aspcf_windows(y1, y2, lo, hi, v1, v2, 6, a.gamma, leg, stats, want_cost=True)
        walls, kernel_ms = [], []
        for it in range(a.warmup + a.repeats):
            t0 = time.perf_counter()
            call()
            if it >= a.warmup:
                walls.append(time.perf_counter() - t0)
                kernel_ms.append(stats.get("kernel_ms", 0.0))
        w = np.array(walls) * 1e3
        n_timed = n_ref if leg == "reference" else a.windows
        rec = dict(tool="aspcf_bench", leg=leg, job=job, windows_timed=n_timed, host_path=stats.get("host_path"), warmup=a.warmup, repeats=a.repeats,
                   call_ms_median=round(float(np.median(w)), 3), call_ms_min=round(float(w.min()), 3), call_ms_max=round(float(w.max()), 3),
                   ms_per_window=round(float(np.median(w)) / n_timed, 4),
                   kernel_ms_median=round(float(np.median(kernel_ms)), 4) if leg == "device" else None,
                   cpus=len(os.sched_getaffinity(0)), interpreter="CPython %s" % sys.version.split()[0])
        print(json.dumps(rec))
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
    if "host" in results and "device" in results:
        (ds, dc), (hs, hc) = results["device"], results["host"]
        if not ((ds == hs).all() and (dc.view(np.uint64) == hc.view(np.uint64)).all()):
            sys.exit("aspcf_bench: the host and device legs differ")
        print("host and device: the same bits")


if __name__ == "__main__":
    main()
