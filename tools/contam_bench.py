"""Times of cto_bam_coverage and cto_bam_mix (what gen_contaminated_bam spends its time in) on synthetic coordinate-sorted long-read BAMs,
a tumour and a normal one per size: per size and entry point the device call and the host path of the same call - wall time around the
call (it ends with the device waited for and the files closed) and the call's own split: copy up + inflate | the kernels (CRC-32 .. gather
or min / max) | the copies down (HIP events) | deflate + write + index (host wall time; the mix only).  The host path reports the reading
of its windows in the first column.  One JSON line per run is appended to profiles/contam_bench.jsonl.
    python tools/contam_bench.py [--region_kb 100 500] [--coverage 30] [--bam_dir DIR] [--repeats 5] [--where device host] [--out FILE]
--bam_dir: reuse (or write, when missing) contam_bench_{t,n}_<kb>.bam there, so that a run on the GPU machine does not spend its time in
Python's zlib.  The reference starts mosdepth and samtools for this step and cannot be timed where there is neither."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--region_kb", type=int, nargs="+", default=[100, 500])
    ap.add_argument("--coverage", type=int, default=30)
    ap.add_argument("--bam_dir", default=None)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host_threads", type=int, default=16)
    ap.add_argument("--purity", type=float, default=0.7, help="the mix keeps this share of the tumour and one minus it of the normal")
    ap.add_argument("--where", nargs="+", default=["device", "host"], choices=["device", "host"])
    ap.add_argument("--write_only", action="store_true", help="write the BAMs and stop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contam_bench.jsonl"))
    a = ap.parse_args()
    bam_dir = a.bam_dir or tempfile.mkdtemp()
    os.makedirs(bam_dir, exist_ok=True)
    out_dir = tempfile.mkdtemp()
    m_t, m_n = int(round(a.purity * 1000)), 1000 - int(round(a.purity * 1000))
    for kb in a.region_kb:
        L = kb * 1000
        bams = {}
        for kind, seed in (("t", 1), ("n", 2)):
            bams[kind] = os.path.join(bam_dir, "contam_bench_%s_%d.bam" % (kind, kb))
            if not os.path.exists(bams[kind]):
                from cal_af_bench import write_synthetic_bam
                t0 = time.perf_counter()
                n = write_synthetic_bam(bams[kind], L, a.coverage, seed=seed)
                print("synthetic BAM: %d reads over %d kb, %.1f MB on disk (written in %.1f s)" % (n, kb, os.path.getsize(bams[kind]) / 1e6,
                                                                                                  time.perf_counter() - t0))
        if a.write_only:
            continue
        from clairs_to_amd.gen_contaminated_bam import bam_coverage, mix_bams
        results = {}
        for where in a.where:
            if where == "device":
                import torch
                if not torch.cuda.is_available():
                    sys.exit("contam_bench: no GPU for --where device")
            for call in ("coverage", "mix"):
                walls, stats, got = [], [], None
                out = os.path.join(out_dir, "mix_%s_%d.bam" % (where, kb))
                for it in range(a.warmup + a.repeats):
                    st = {}
                    t0 = time.perf_counter()
                    if call == "coverage":
                        got = bam_coverage(bams["t"], where=where, host_threads=a.host_threads, stats=st)
                    else:
                        got = mix_bams(bams["t"], bams["n"], out, m_t, m_n, where=where, host_threads=a.host_threads, stats=st)
                    if it >= a.warmup:
                        walls.append(time.perf_counter() - t0)
                        stats.append(st)
                if call == "mix":
                    with open(out, "rb") as f, open(out + ".bai", "rb") as g:
                        got = (got, f.read(), g.read())
                w = np.array(walls)
                s0 = stats[len(stats) // 2]
                ms = lambda k: round(float(np.median([s[k] for s in stats])), 3)
                rec = dict(tool="contam_bench", call=call, where=where, region_kb=kb, coverage=a.coverage,
                           bam_mb=[round(os.path.getsize(bams[k]) / 1e6, 2) for k in (("t",) if call == "coverage" else ("t", "n"))],
                           host_threads=a.host_threads, warmup=a.warmup, repeats=a.repeats, wall_s_median=round(float(np.median(w)), 5),
                           wall_s_min=round(float(w.min()), 5), wall_s_max=round(float(w.max()), 5), n_chunks=int(s0["n_chunks"]),
                           n_records=int(s0["n_records"]), fallback_chunks=int(s0["fallback_chunks"]), inflated_mb=round(s0["inflated_bytes"] / 1e6, 2),
                           ms_copy_up_inflate=ms("ms_inflate"), ms_kernels=ms("ms_kernels"), ms_copy_down=ms("ms_copy"), ms_deflate_write=ms("ms_write"))
                if call == "mix":
                    rec.update(m_tumor=m_t, m_normal=m_n, kept=s0["kept"], candidates=s0["candidates"], out_mb_inflated=round(s0["out_bytes"] / 1e6, 2),
                               out_mb=round(len(got[1]) / 1e6, 2))
                else:
                    rec.update(mean_depth=round(got[0]["bases"] / got[0]["length"], 2), max_depth=got[0]["max"])
                results[where, call] = got
                print(json.dumps(rec))
                os.makedirs(os.path.dirname(a.out), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")
        for call in ("coverage", "mix"):
            if ("device", call) in results and ("host", call) in results and results["device", call] != results["host", call]:
                sys.exit("contam_bench: device and host differ in %s" % call)


if __name__ == "__main__":
    main()
