"""Throughput of the allele counter (cto_allele_counts) on a synthetic coordinate-sorted long-read BAM of the kind tools/bam_bench.py
writes, loci at the 1000-Genomes density of about one per 230 bp: loci/s, reads/s, inflated GB/s and the three stage times for the
device path and for the host path at 16 threads.  One JSON line per run is appended to profiles/allele_bench.jsonl.
    python tools/allele_bench.py [--region_kb 400] [--coverage 30] [--bam FILE] [--repeats 5] [--where device host] [--out FILE]
--bam: reuse (or write, when missing) this BAM, so that a run on the GPU machine does not spend its time in Python's zlib."""
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


def write_synthetic_bam(bam, L, cov, seed=1):
    from bamutil import write_bam
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    ref = acgt[rng.integers(0, 4, size=L)]
    reads, bases, i = [], 0, 0
    while bases < cov * L:
        n = int(np.clip(rng.lognormal(9.0, 0.5), 1000, 30000))
        pos = int(rng.integers(0, max(1, L - n)))
        n = min(n, L - pos)
        seg = ref[pos:pos + n].copy()
        mm = rng.random(n) < 0.01
        seg[mm] = acgt[rng.integers(0, 4, size=int(mm.sum()))]
        cigar, seq, rp = [], [], 0                                  # one insertion / deletion every ~30 bases, as ONT CIGARs have
        cuts = np.sort(rng.choice(np.arange(10, max(11, n - 10)), size=max(1, n // 30), replace=False)) if n > 40 else []
        for c in cuts:
            if c - rp <= 0:
                continue
            cigar.append(("M", int(c - rp)))
            seq.append(seg[rp:c])
            rp = int(c)
            if rng.random() < 0.4:
                k = int(rng.integers(1, 4))
                cigar.append(("I", k))
                seq.append(acgt[rng.integers(0, 4, size=k)])
            else:
                k = int(min(rng.integers(1, 4), n - rp - 1))
                if k > 0:
                    cigar.append(("D", k))
                    rp += k
        if n - rp > 0:
            cigar.append(("M", int(n - rp)))
            seq.append(seg[rp:n])
        s = np.concatenate(seq)
        q = np.clip(np.rint(rng.normal(28, 8, size=s.size)), 1, 50).astype(np.uint8)
        reads.append(dict(name="r%d" % i, flag=16 * int(rng.random() < 0.5), ref=0, pos=pos, mapq=60, cigar=cigar, seq=s.tobytes().decode(), qual=q.tolist()))
        bases += n
        i += 1
    reads.sort(key=lambda r: r["pos"])
    write_bam(bam, [("chr1", L)], reads, block_payload=65000)
    return len(reads)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--region_kb", type=int, default=400)
    ap.add_argument("--coverage", type=float, default=30.0)
    ap.add_argument("--bam", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host_threads", type=int, default=16)
    ap.add_argument("--where", nargs="+", default=["device", "host"], choices=["device", "host"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "allele_bench.jsonl"))
    a = ap.parse_args()
    L = a.region_kb * 1000
    bam = a.bam or os.path.join(tempfile.mkdtemp(), "allele_bench.bam")
    if not os.path.exists(bam):
        t0 = time.perf_counter()
        n = write_synthetic_bam(bam, L, a.coverage)
        print("synthetic BAM: %d reads over %d kb, %.1f MB on disk (written in %.1f s)" % (n, a.region_kb, os.path.getsize(bam) / 1e6, time.perf_counter() - t0))
    from clairs_to_amd.allele_counter import count_alleles
    rng = np.random.default_rng(7)
    loci = np.unique(rng.integers(1, L + 1, size=L // 230))
    results = {}
    for where in a.where:
        if where == "device":
            import torch
            if not torch.cuda.is_available():
                sys.exit("allele_bench: no GPU for --where device")
        walls, stats, counts = [], [], None
        for it in range(a.warmup + a.repeats):
            st = {}
            t0 = time.perf_counter()
            counts = count_alleles(bam, "chr1", loci, min_bq=20, min_mq=20, req_flags=0, excl_flags=2316, where=where, host_threads=a.host_threads, stats=st)
            if it >= a.warmup:
                walls.append(time.perf_counter() - t0)
                stats.append(st)
        w = np.array(walls)
        med = float(np.median(w))
        s0 = stats[len(stats) // 2]
        rec = dict(tool="allele_bench", where=where, region_kb=a.region_kb, coverage=a.coverage, bam_mb=round(os.path.getsize(bam) / 1e6, 2), n_loci=int(len(loci)),
                   host_threads=a.host_threads if where == "host" else None, warmup=a.warmup, repeats=a.repeats, wall_s_median=round(med, 5),
                   wall_s_min=round(float(w.min()), 5), wall_s_max=round(float(w.max()), 5), loci_per_s=round(len(loci) / med, 1),
                   reads_per_s=round(s0["n_reads_entered"] / med, 1), n_chunks=int(s0["n_chunks"]), n_reads_entered=int(s0["n_reads_entered"]),
                   fallback_chunks=int(s0["fallback_chunks"]), inflated_mb=round(s0["inflated_bytes"] / 1e6, 2),
                   inflated_gb_per_s=round(s0["inflated_bytes"] / med / 1e9, 3) if s0["inflated_bytes"] else None,
                   ms_inflate=round(float(np.median([s["ms_inflate"] for s in stats])), 3), ms_records=round(float(np.median([s["ms_records"] for s in stats])), 3),
                   ms_count=round(float(np.median([s["ms_count"] for s in stats])), 3), total_counted=int(counts.sum()))
        results[where] = counts
        print(json.dumps(rec))
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
    if len(results) == 2 and not np.array_equal(results["device"], results["host"]):
        sys.exit("allele_bench: device and host counts differ")


if __name__ == "__main__":
    main()
