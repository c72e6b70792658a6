#!/usr/bin/env python3
"""Panel-of-normals scan benchmark (nonsomatic_tagging, csrc/pon.hip).

Writes a seeded gnomAD-like BGZF PoN (24 contigs, ~300-byte INFO fields; --records sets the size: the default 15.4 M records are about 1 GB compressed) with
a .tbi, and 100 k calls drawn from it, then reports
  device   (a) the device scan of the whole file and of one contig through the .tbi: GB/s of inflated text, records/s;
           (b) the mirror's wall time per invocation (call set up, scan, md5 on its host thread) with and without the md5;
  reference (c) src/nonsomatic_tagging.py:_apply_pon_streaming on the same file on this host's CPU (CPython with the system gzip, not the
           PyPy run_clairs_to uses; no tabix: its full-stream path).
Device measurements are warmed up once, then repeated --reps times; the reference leg (a 30-s pass with nothing to warm) is repeated
--reps times.  Spread: median, min, max.  One JSON object per mode is appended to --out.
  python tools/pon_bench.py device --dir /tmp/pon --out profiles/pon_bench.jsonl
  python tools/pon_bench.py reference --ref-src <checkout of the reference> --dir /tmp/pon --out profiles/pon_bench.jsonl"""
import argparse
import json
import os
import statistics
import struct
import sys
import time
from multiprocessing import Pool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONTIGS = ["chr%d" % i for i in range(1, 23)] + ["chrX", "chrY"]
HEADER = b"##fileformat=VCFv4.2\n##source=pon_bench\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"


def contig_text(args):
    """one contig's records (deterministic in seed and contig index), BGZF-compressed; -> (bytes, first POS list sample for the calls)"""
    import numpy as np
    from ponutil import bgzf_block
    ci, n, seed = args
    rng = np.random.default_rng(seed * 1000 + ci)
    pos = np.cumsum(rng.integers(1, 60, n))
    ref = np.array(list("ACGT"))[rng.integers(0, 4, n)]
    alts = np.array(["A", "C", "G", "T", "AT", "C,G", "G,T,A"])[rng.integers(0, 7, n)]
    af = rng.integers(1, 10 ** 6, n)
    ac = rng.integers(1, 5000, n)
    ctg = CONTIGS[ci]
    lines = ["%s\t%d\trs%d\t%s\t%s\t%d.00\tPASS\tAC=%d;AN=251000;AF=%.6e;nhomalt=%d;AC_afr=%d;AF_afr=%.4e;AC_amr=%d;AC_eas=%d;AC_nfe=%d;vep=%s|%s|MODIFIER|GENE%d|ENSG%011d|Transcript|ENST%011d|intron_variant;popmax=nfe;faf95=%.3e\n"
             % (ctg, p, p * 7 + ci, r, a, q, c, f / 1e9, c // 7, c // 3, f / 3e9, c // 5, c // 11, c // 2, a, "intron", p % 4000, p // 97,
                p // 89, f / 7e9)
             for p, r, a, q, c, f in zip(pos.tolist(), ref.tolist(), alts.tolist(), (af % 900).tolist(), ac.tolist(), af.tolist())]
    text = "".join(lines).encode()
    out = [bgzf_block(text[u:u + 65280], 1) for u in range(0, len(text), 65280)]
    pick = rng.choice(n, size=max(1, 100000 // len(CONTIGS)), replace=False)
    calls = [(ctg, int(pos[i]), str(ref[i]) if rng.random() < 0.8 else "T", str(alts[i]).split(",")[0]) for i in pick]
    return b"".join(out), len(text), calls


def write_pon(d, n_records, seed):
    from ponutil import bgzf_block, BGZF_EOF
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, "pon_bench.vcf.gz")
    per = n_records // len(CONTIGS)
    with Pool(16) as pool:
        parts = pool.map(contig_text, [(i, per, seed) for i in range(len(CONTIGS))])
    head = bgzf_block(HEADER, 1)
    names, offs, calls, text_bytes = [], [], [], len(HEADER)
    with open(path, "wb") as f:
        f.write(head)
        c = len(head)
        for ci, (comp, nt, cs) in enumerate(parts):
            offs.append((c, c + len(comp)))
            f.write(comp)
            c += len(comp)
            text_bytes += nt
            calls += cs
        f.write(BGZF_EOF)
    # the index: each contig starts a block; one chunk in bin 0 covers it (valid for the whole-contig reads measured here)
    raw = [b"TBI\x01", struct.pack("<iiiiiiii", len(CONTIGS), 2, 1, 2, 0, ord("#"), 0, sum(len(n) + 1 for n in CONTIGS)),
           b"".join(n.encode() + b"\0" for n in CONTIGS)]
    for b, e in offs:
        raw.append(struct.pack("<iIiQQ", 1, 0, 1, b << 16, e << 16) + struct.pack("<iQ", 1, b << 16))
    with open(path + ".tbi", "wb") as f:
        f.write(bgzf_block(b"".join(raw)) + BGZF_EOF)
    with open(os.path.join(d, "calls.json"), "w") as f:
        json.dump(calls[:100000], f)
    return path, text_bytes


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def device(a):
    import torch
    from clairs_to_amd.nonsomatic_tagging import PonScanner, pon_hits
    path, text_bytes = write_pon(a.dir, a.records, a.seed)
    calls = json.load(open(os.path.join(a.dir, "calls.json")))
    sets, one = {}, {}
    for c, p, r, al in calls:
        sets.setdefault(c, {})[p] = dict(ref=r, alt=al)
    one = {"chr2": sets["chr2"]}
    torch.cuda.init()
    res = dict(mode="device", file_bytes=os.path.getsize(path), text_bytes=text_bytes, records=a.records // len(CONTIGS) * len(CONTIGS),
               calls=len(calls), device=torch.cuda.get_device_name(0))
    for label, s, only in (("whole_file", sets, None), ("one_contig_tbi", one, "chr2")):
        sc = PonScanner(s)
        ts, st = [], None
        for r in range(a.reps + 1):
            t0 = time.perf_counter()
            hits, st, host = sc.match(path, only, True)
            dt = time.perf_counter() - t0
            if r:
                ts.append(dt)
        sc.close()
        res[label] = dict(seconds=spread(ts), inflated_GBps=st.bytes_inflated / statistics.median(ts) / 1e9,
                          records_per_s=st.records / statistics.median(ts), bytes_read=st.bytes_read, bytes_inflated=st.bytes_inflated,
                          blocks=st.blocks_device, used_tbi=st.used_tbi, hits=len(hits), host_lines=len(host))
    for label, skip in (("invocation_md5", False), ("invocation_skip_md5", True)):    # what one contig invocation of the mirror spends
        ts = []
        for r in range(a.reps + 1):
            t0 = time.perf_counter()
            sc = PonScanner(one)
            pon_hits(sc, path, "chr2", True, one, skip)
            sc.close()
            if r:
                ts.append(time.perf_counter() - t0)
        res[label] = dict(seconds=spread(ts))
    return res


def reference(a):
    sys.path.insert(0, a.ref_src)
    from collections import defaultdict
    from src.nonsomatic_tagging import _apply_pon_streaming, _build_input_ids_by_contig_pos
    path, text_bytes = write_pon(a.dir, a.records, a.seed)
    calls = json.load(open(os.path.join(a.dir, "calls.json")))
    pos_set, id_set = defaultdict(set), defaultdict(set)
    for c, p, r, al in calls:
        if c == "chr2":
            pos_set[c].add(str(p))
            id_set[c].add("%d\t%s\t%s" % (p, r, al))
    ids_by_pos = _build_input_ids_by_contig_pos(id_set)
    ts = []
    for r in range(a.reps):
        filt = {k: set(v) for k, v in id_set.items()}
        t0 = time.perf_counter()
        _apply_pon_streaming(path, "chr2", list(id_set), True, pos_set, id_set, ids_by_pos, filt, skip_pon_md5=False)
        ts.append(time.perf_counter() - t0)
    return dict(mode="reference", interpreter="CPython %s" % sys.version.split()[0], path="full stream (no tabix)",
                file_bytes=os.path.getsize(path), text_bytes=text_bytes, one_contig_invocation_seconds=spread(ts),
                inflated_GBps=text_bytes / statistics.median(ts) / 1e9)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("mode", choices=("device", "reference"))
    p.add_argument("--dir", required=True)
    p.add_argument("--records", type=int, default=15400000)
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--ref-src", default=None)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    res = device(a) if a.mode == "device" else reference(a)
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
