"""Times of the phasing engine (cto_phase_reads, what phase_tumor spends its device time in) on synthetic coordinate-sorted long-read
BAMs (clairs_to_amd.synth_run.make_bam_run), sites at one per --spacing bases with the reference's letter as REF: per size the device
call (wall time, and by HIP events: copy up + inflate | the record front end | the observation, link and assignment kernels | the copies
down and the merged reads' copy up; the phase pass on the host by the wall clock) and the host path of the same call.  One JSON line per
run is appended to profiles/phase_bench.jsonl.  No speed bar: both paths are reported as they come out.
    python tools/phase_bench.py [--region_kb 100 500] [--depth 30] [--spacing 1000] [--bam_dir DIR] [--repeats 5] [--where device host]
--bam_dir: reuse (or write, when missing) phase_bench_<kb>/ there, so that a run on the GPU machine does not spend its time writing BAMs."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sites_of(run, spacing, seed=3):
    with open(run["ref_fn"]) as f:
        ref = "".join(ln.strip() for ln in f if not ln.startswith(">"))
    rng = np.random.default_rng(seed)
    pos = list(range(500, len(ref) - 500, spacing))
    refs = [ref[p - 1] for p in pos]
    alts = ["ACGT"[("ACGT".index(r) + 1 + int(rng.integers(0, 3))) % 4] for r in refs]
    return pos, refs, alts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--region_kb", type=int, nargs="+", default=[100, 500])
    ap.add_argument("--depth", type=int, default=30)
    ap.add_argument("--spacing", type=int, default=1000)
    ap.add_argument("--link_span", type=int, default=8)
    ap.add_argument("--bam_dir", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host_threads", type=int, default=16)
    ap.add_argument("--where", nargs="+", default=["device", "host"], choices=["device", "host"])
    ap.add_argument("--write_only", action="store_true", help="write the BAMs and stop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phase_bench.jsonl"))
    a = ap.parse_args()
    bam_dir = a.bam_dir or tempfile.mkdtemp()
    from clairs_to_amd.synth_run import make_bam_run
    for kb in a.region_kb:
        d = os.path.join(bam_dir, "phase_bench_%d" % kb)
        run = dict(ref_fn=os.path.join(d, "ref.fa"), bam_fn=os.path.join(d, "tumor.bam"), ctg="chr1")
        if not os.path.exists(run["bam_fn"]):
            t0 = time.perf_counter()
            run = make_bam_run(d, region_kb=kb, n_chunks=1, depth=a.depth, seed=kb)
            print("synthetic BAM: %d kb at %dx, %.1f MB on disk (written in %.1f s)" % (kb, a.depth, os.path.getsize(run["bam_fn"]) / 1e6, time.perf_counter() - t0))
        if a.write_only:
            continue
        from clairs_to_amd.phase_tumor import phase_reads
        pos, refs, alts = sites_of(run, a.spacing)
        results = {}
        for where in a.where:
            if where == "device":
                import torch
                if not torch.cuda.is_available():
                    sys.exit("phase_bench: no GPU for --where device")
            walls, stats, got = [], [], None
            for it in range(a.warmup + a.repeats):
                st = {}
                t0 = time.perf_counter()
                got = phase_reads(run["bam_fn"], run["ctg"], pos, refs, alts, link_span=a.link_span, where=where, host_threads=a.host_threads, stats=st)
                if it >= a.warmup:
                    walls.append(time.perf_counter() - t0)
                    stats.append(st)
            w = np.array(walls)
            s0 = stats[len(stats) // 2]
            ms = lambda k: round(float(np.median([s[k] for s in stats])), 3)
            rec = dict(tool="phase_bench", where=where, region_kb=kb, depth=a.depth, bam_mb=round(os.path.getsize(run["bam_fn"]) / 1e6, 2), n_sites=len(pos),
                       link_span=a.link_span, host_threads=a.host_threads if where == "host" else None, warmup=a.warmup, repeats=a.repeats,
                       wall_s_median=round(float(np.median(w)), 5), wall_s_min=round(float(w.min()), 5), wall_s_max=round(float(w.max()), 5),
                       n_chunks=int(s0["n_chunks"]), n_reads=int(len(got["voff"])), n_obs=int(len(got["obs"])), n_merged_reads=int(s0["n_merged_reads"]),
                       fallback_chunks=int(s0["fallback_chunks"]), inflated_mb=round(s0["inflated_bytes"] / 1e6, 2), n_phase_blocks=int(s0["n_phase_blocks"]),
                       ms_copy_up_inflate=ms("ms_inflate"), ms_records=ms("ms_records"), ms_kernels=ms("ms_count"), ms_copy_down=ms("ms_copy"),
                       ms_phase_pass=ms("ms_phase"), n_tagged=int((got["hp"] > 0).sum()), n_phased=int((got["phase"] >= 0).sum()))
            results[where] = got
            print(json.dumps(rec))
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")
        if len(results) == 2 and not all(np.array_equal(results["device"][k], results["host"][k]) for k in results["host"]):
            sys.exit("phase_bench: device and host results differ")


if __name__ == "__main__":
    main()
