"""Throughput of the AF tallies (cto_af_tallies, what cal_af_distribution spends its time in) on synthetic coordinate-sorted long-read
BAMs with HP tags, truth variants at about one per 500 bp (four SNVs to one insertion or deletion): per size the device call (wall time,
and the HIP-event times of its three stages: copy up + inflate | records | HP classes, tally, copy down) and the host path of the same
call.  One JSON line per run is appended to profiles/cal_af_bench.jsonl.
    python tools/cal_af_bench.py [--region_kb 100 400] [--coverage 30] [--bam_dir DIR] [--repeats 5] [--where device host] [--out FILE]
--bam_dir: reuse (or write, when missing) cal_af_bench_<kb>.bam there, so that a run on the GPU machine does not spend its time in
Python's zlib.  The reference itself starts one samtools process per variant and cannot be timed where there is no samtools."""
import argparse
import json
import os
import struct
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def write_synthetic_bam(bam, L, cov, seed=1):
    """reads of about 8 kb with an insertion or deletion every ~30 bases, a reference skip in one read of fifty, HP 1 / 2 / absent"""
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
        cigar, seq, rp = [], [], 0
        cuts = np.sort(rng.choice(np.arange(10, max(11, n - 10)), size=max(1, n // 30), replace=False)) if n > 40 else []
        skip_at = int(rng.integers(0, len(cuts))) if len(cuts) and rng.random() < 0.02 else -1
        for ci, c in enumerate(cuts):
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
                    cigar.append(("N" if ci == skip_at else "D", k))
                    rp += k
        if n - rp > 0:
            cigar.append(("M", int(n - rp)))
            seq.append(seg[rp:n])
        s = np.concatenate(seq)
        q = np.clip(np.rint(rng.normal(28, 8, size=s.size)), 1, 50).astype(np.uint8)
        hp = int(rng.integers(0, 3))
        aux = b"NMi" + struct.pack("<i", 5) + b"MDZ" + b"100A20" + b"\0" + (b"HPC" + bytes([hp]) if hp else b"") + b"PSi" + struct.pack("<i", pos)
        reads.append(dict(name="r%d" % i, flag=16 * int(rng.random() < 0.5), ref=0, pos=pos, mapq=60, cigar=cigar, seq=s.tobytes().decode(), qual=q.tolist(),
                          aux=aux))
        bases += n
        i += 1
    reads.sort(key=lambda r: r["pos"])
    write_bam(bam, [("chr1", L)], reads, block_payload=65000)
    return len(reads)


def truth_alleles(L, seed=7):
    from clairs_to_amd.cal_af_distribution import KIND_DEL, KIND_INS, KIND_SNV
    rng = np.random.default_rng(seed)
    loci = np.unique(rng.integers(1, L + 1, size=L // 500))
    alleles = []
    for _ in loci:
        x, b = rng.random(), "ACGT"[int(rng.integers(0, 4))]
        if x < 0.8:
            alleles.append((KIND_SNV, b, 0, b""))
        elif x < 0.9:
            alleles.append((KIND_INS, b, 0, bytes(rng.choice(list(b"ACGT"), size=int(rng.integers(1, 4))).tolist())))
        else:
            alleles.append((KIND_DEL, b, int(rng.integers(1, 4)), b""))
    return loci, alleles


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--region_kb", type=int, nargs="+", default=[100, 400])
    ap.add_argument("--coverage", type=float, default=30.0)
    ap.add_argument("--bam_dir", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host_threads", type=int, default=16)
    ap.add_argument("--where", nargs="+", default=["device", "host"], choices=["device", "host"])
    ap.add_argument("--write_only", action="store_true", help="write the BAMs and stop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cal_af_bench.jsonl"))
    a = ap.parse_args()
    bam_dir = a.bam_dir or tempfile.mkdtemp()
    os.makedirs(bam_dir, exist_ok=True)
    for kb in a.region_kb:
        L = kb * 1000
        bam = os.path.join(bam_dir, "cal_af_bench_%d.bam" % kb)
        if not os.path.exists(bam):
            t0 = time.perf_counter()
            n = write_synthetic_bam(bam, L, a.coverage)
            print("synthetic BAM: %d reads over %d kb, %.1f MB on disk (written in %.1f s)" % (n, kb, os.path.getsize(bam) / 1e6, time.perf_counter() - t0))
        if a.write_only:
            continue
        from clairs_to_amd.cal_af_distribution import tally
        loci, alleles = truth_alleles(L)
        results = {}
        for where in a.where:
            if where == "device":
                import torch
                if not torch.cuda.is_available():
                    sys.exit("cal_af_bench: no GPU for --where device")
            walls, stats, got = [], [], None
            for it in range(a.warmup + a.repeats):
                st = {}
                t0 = time.perf_counter()
                got = tally(bam, "chr1", loci, alleles, where=where, host_threads=a.host_threads, stats=st)
                if it >= a.warmup:
                    walls.append(time.perf_counter() - t0)
                    stats.append(st)
            w = np.array(walls)
            med = float(np.median(w))
            s0 = stats[len(stats) // 2]
            ms = lambda k: round(float(np.median([s[k] for s in stats])), 3)
            rec = dict(tool="cal_af_bench", where=where, region_kb=kb, coverage=a.coverage, bam_mb=round(os.path.getsize(bam) / 1e6, 2), n_loci=int(len(loci)),
                       host_threads=a.host_threads if where == "host" else None, warmup=a.warmup, repeats=a.repeats, wall_s_median=round(med, 5),
                       wall_s_min=round(float(w.min()), 5), wall_s_max=round(float(w.max()), 5), loci_per_s=round(len(loci) / med, 1),
                       n_chunks=int(s0["n_chunks"]), n_reads_entered=int(s0["n_reads_entered"]), fallback_chunks=int(s0["fallback_chunks"]),
                       host_loci=int(s0["host_loci"]), inflated_mb=round(s0["inflated_bytes"] / 1e6, 2), ms_inflate=ms("ms_inflate"), ms_records=ms("ms_records"),
                       ms_count=ms("ms_count"), kernel_ms=round(ms("ms_inflate") + ms("ms_records") + ms("ms_count"), 3) if where == "device" else None,
                       depth_sum=int(got[:, 0].sum()), alt_sum=int(got[:, 1].sum()))
            results[where] = got
            print(json.dumps(rec))
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")
        if len(results) == 2 and not np.array_equal(results["device"], results["host"]):
            sys.exit("cal_af_bench: device and host tallies differ")


if __name__ == "__main__":
    main()
