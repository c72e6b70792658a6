#!/usr/bin/env python3
"""Calls per second of cto_postfilter_windows (csrc/postfilter.hip) on a generated Illumina-like job set: `--contigs` simulated contigs of
`--length` bp at `--depth`x (tests/golden/pfsim.py), a call every `--every` bp, cut into jobs of 256 calls as the module does.  Prints and
appends to profiles/postfilter_bench.jsonl: the packer's rate (host), the C call's rate (upload + kernel + download) and the kernel's own
time from HIP events, with the algorithmic bytes of the packed windows (8 bytes per read-base of every window) against HBM bandwidth.
Usage: python tools/postfilter_bench.py [--contigs 4] [--length 20000] [--depth 60] [--every 20] [--repeat 5]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

HBM_BYTES_PER_S = 8.0e12            # MI355X peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=4)
    ap.add_argument("--length", type=int, default=20000)
    ap.add_argument("--depth", type=int, default=60)
    ap.add_argument("--every", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import pfsim
    from clairs_to_amd.haplotype_filtering import partition_jobs
    from clairs_to_amd.postfilter_variants import PackedJob, evaluate_windows
    texts, calls = [], []
    for k in range(a.contigs):
        sim = pfsim.simulate(1000 + k, length=a.length, depth=a.depth)
        pos = list(range(150, a.length - 150, a.every))
        for lo, hi, ps in partition_jobs(pos, 100, 256, 50000):
            texts.append((pfsim.pileup_text(sim, "c%d" % k, range(lo, hi + 1)), sim["ref"][lo - 1:hi], lo))
            calls += [(len(texts) - 1, p, sim["ref"][p - 1], pfsim.other(sim["ref"][p - 1], 2)) for p in ps]
    t0 = time.time()
    jobs = [PackedJob(t, r, lo, 100) for t, r, lo in texts]
    pack_s = time.time() - t0
    window_names = 0
    for j, job in enumerate(jobs):
        v = job.view()
        csum = np.concatenate([[0], np.cumsum(np.diff(v["col_off"]))])
        for c in calls:
            if c[0] == j:
                i0, i1 = np.searchsorted(v["col_pos"], [max(c[1] - 100, 1), c[1] + 100 + 1])
                window_names += int(csum[i1] - csum[i0])
    evaluate_windows(jobs, calls)                               # warm-up: buffers, code object
    best_call, best_kernel = 1e9, 1e9
    for _ in range(a.repeat):
        t0 = time.time()
        out, ms = evaluate_windows(jobs, calls, want_kernel_ms=True)
        best_call, best_kernel = min(best_call, time.time() - t0), min(best_kernel, ms / 1e3)
    bytes_alg = 8.0 * window_names
    rec = dict(bench="postfilter_windows", calls=len(calls), jobs=len(jobs), depth=a.depth, text_mb=round(sum(len(t[0]) for t in texts) / 1e6, 2),
               host_path_calls=int((out[:, 9] == 1).sum()), pack_calls_per_s=round(len(calls) / pack_s, 1),
               c_call_calls_per_s=round(len(calls) / best_call, 1), kernel_ms=round(best_kernel * 1e3, 4),
               kernel_calls_per_s=round(len(calls) / best_kernel, 1), window_read_bases=window_names, algorithmic_gb=round(bytes_alg / 1e9, 4),
               kernel_gb_per_s=round(bytes_alg / best_kernel / 1e9, 1), hbm_floor_ms=round(bytes_alg / HBM_BYTES_PER_S * 1e3, 4))
    print(json.dumps(rec))
    with open(os.path.join(ROOT, "profiles", "postfilter_bench.jsonl"), "a") as f:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
