"""Throughput of the haplotype filter's job producers on hapsim contigs (tests/golden/hapsim.py, the load of bench.py's
hapfilter.many_calls: 216 contigs, every call of the SNV pass): the nine-column text path (cto_hap_job_from_text on prepared text,
no samtools in the loop), the BAM host path and the BAM device path of cto_hap_windows, each followed by cto_hap_evaluate.  One JSON
line per configuration is appended to profiles/hap_windows_bench.jsonl: calls/s and the split of a job - read, copy up + inflate,
records, kernels, copy down, job build, evaluate.
    python tools/hap_windows_bench.py [--contigs 216] [--work_dir DIR] [--paths text host device] [--repeats 3] [--out FILE]
--work_dir: reuse (or write, when missing) the contigs' BAMs, texts and calls there, so that a run on the GPU machine does not spend
its time in Python.  `--prepare` only writes them.  The device path runs in a child process under its own time limit."""
import argparse
import json
import os
import pickle
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def prepare(work_dir, n_contigs):
    import bamutil
    import haputil
    import hapsim
    import gen_hapfilter_wide as gw
    os.makedirs(work_dir, exist_ok=True)
    for k in range(n_contigs):
        fn = os.path.join(work_dir, "c%d.pkl" % k)
        if os.path.exists(fn):
            continue
        ctg = "ctg%d" % k
        sim = hapsim.simulate(seed=1000 + k)
        vcf, text = gw.inputs_for(sim, ctg, "snv")
        bam = os.path.join(work_dir, "c%d.bam" % k)
        bamutil.write_bam(bam, [(ctg, len(sim["ref"]))], haputil.reads_of(sim), block_payload=60000, level=6)
        calls = []
        for row in vcf.split("\n"):
            c = row.split("\t")
            if row and row[0] != "#" and c[6] == "PASS":
                calls.append((int(c[1]), c[3], c[4], float(c[9].split(":")[3]), "", ""))
        with open(fn, "wb") as f:
            pickle.dump(dict(ctg=ctg, ref=sim["ref"], text=text, calls=calls, bam=bam), f)


def run(work_dir, n_contigs, path, repeats):
    from clairs_to_amd.haplotype_filtering import HapJob, flank_bed
    jobs = []
    for k in range(n_contigs):
        with open(os.path.join(work_dir, "c%d.pkl" % k), "rb") as f:
            jobs.append(pickle.load(f))
    best = None
    for _ in range(repeats):
        t_prod = t_eval = 0.0
        stats, n_calls, n_recs, text_bytes = {}, 0, 0, 0
        t0 = time.perf_counter()
        for j in jobs:
            ps = [c[0] for c in j["calls"]]
            lo, hi = max(1, ps[0] - 100), ps[-1] + 101
            a = time.perf_counter()
            if path == "text":
                job = HapJob.from_text(j["text"], lo, hi)
                text_bytes += len(j["text"])
            else:
                job = HapJob.from_bam(j["bam"], j["ctg"], lo, hi, flank_bed(ps, 100), reverse_del=True, where=path)
                for key, v in job.stats.items():
                    stats[key] = stats.get(key, 0) + v
            b = time.perf_counter()
            job.evaluate(j["ref"][lo - 1:hi], lo, j["calls"], 100, 2, False)
            t_eval += time.perf_counter() - b
            t_prod += b - a
            n_calls += len(ps)
            job.close()
        wall = time.perf_counter() - t0
        rec = dict(path=path, contigs=n_contigs, calls=n_calls, wall_s=round(wall, 4), calls_per_s=round(n_calls / wall, 1),
                   produce_s=round(t_prod, 4), evaluate_s=round(t_eval, 4), text_mb=round(text_bytes / 1e6, 1))
        for key in ("ms_read", "ms_inflate", "ms_records", "ms_kernels", "ms_down", "ms_build"):
            if key in stats:
                rec[key] = round(stats[key], 2)
        for key in ("n_recs", "n_reads_entered", "fallback_chunks", "cap_chunks", "host_columns", "inflated_bytes"):
            if key in stats:
                rec[key] = int(stats[key])
        if best is None or rec["wall_s"] < best["wall_s"]:
            best = rec
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=216)
    ap.add_argument("--work_dir", default=os.path.join(tempfile.gettempdir(), "hap_windows_bench"))
    ap.add_argument("--paths", nargs="+", default=["text", "host", "device"], choices=["text", "host", "device"])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--prepare", action="store_true")
    ap.add_argument("--timeout", type=int, default=300, help="seconds for the child process of the device path")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hap_windows_bench.jsonl"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(run(a.work_dir, a.contigs, a.child, a.repeats)), flush=True)
        return
    prepare(a.work_dir, a.contigs)
    if a.prepare:
        return
    for path in a.paths:
        if path == "device":          # a GPU step: a fresh process under its own time limit; nothing more is started after a failure
            res = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "device", "--contigs",
                                  str(a.contigs), "--work_dir", a.work_dir, "--repeats", str(a.repeats)], stdout=subprocess.PIPE)
            if res.returncode != 0:
                sys.exit("device path: exit %d" % res.returncode)
            rec = json.loads([ln for ln in res.stdout.decode().split("\n") if ln.startswith("RESULT ")][-1][7:])
        else:
            rec = run(a.work_dir, a.contigs, path, a.repeats)
        line = json.dumps(rec)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
