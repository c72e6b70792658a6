"""What the BGZF coder on the device (csrc/deflate.hip) costs and saves in gen_contaminated_bam's mix, on the synthetic BAMs of
tools/contam_bench.py (a 30x tumour and a 30x normal per region size).  One JSON line per measurement is appended to
profiles/deflate_bench.jsonl.

  ratio     the size of the mix's blocks from the device coder, and from zlib level 1 and level 6 on the same blocks
  time      per --deflate choice and thread count: the mix on the device, every repeat's ms_write + ms_copy (deflate + write + index on the
            host, and the copies down) and the coder's kernels, with the spread over the repeats.  --parent_root DIR runs the same mix
            from another checkout of the package (the parent commit, built there) in a process of its own, for the comparison
  variants  --variants: the host restatement built with other segment lengths and probe sets (tools/deflate_ratio.cpp, g++), sizes only

    python tools/deflate_bench.py [--region_kb 100 500] [--bam_dir DIR] [--repeats 7] [--threads 16 2] [--parent_root DIR] [--variants]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = [(512, "1,2,3,4,6,8"), (1024, "1,2,3,4,6,8"), (256, "1,2,3,4,6,8"), (512, "1"), (512, "1,2,3,4"), (512, "1,2,3,4,6,8,12,16,24,32")]


def worker(a):
    """the mix, repeated, from the package under a.root -> one JSON line of per-repeat stats"""
    sys.path.insert(0, a.root)
    from clairs_to_amd.gen_contaminated_bam import mix_bams
    out = os.path.join(tempfile.mkdtemp(), "mix.bam")
    reps = []
    for it in range(a.warmup + a.repeats):
        st, dst = {}, {}
        kw = {} if a.deflate == "parent" else dict(deflate=a.deflate, deflate_stats=dst)
        t0 = time.perf_counter()
        mix_bams(a.tumor, a.normal, out, 700, 300, where="device", host_threads=a.host_threads, stats=st, **kw)
        wall = time.perf_counter() - t0
        if it >= a.warmup:
            reps.append(dict(wall_ms=wall * 1e3, ms_write=st["ms_write"], ms_copy=st["ms_copy"], ms_kernels=st["ms_kernels"], ms_inflate=st["ms_inflate"],
                             ms_deflate_kernels=dst.get("ms_kernels", 0.0), fallback=int(st["fallback_chunks"])))
    print("RESULT " + json.dumps(dict(reps=reps, out_bytes=os.path.getsize(out), stream_bytes=int(st["out_bytes"]), out=out,
                                      types=[int(dst.get(k, 0)) for k in ("stored", "fixed", "dynamic")])))


def run_worker(root, deflate, tumor, normal, threads, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--deflate", deflate, "--tumor", tumor, "--normal", normal,
           "--host_threads", str(threads), "--warmup", str(a.warmup), "--repeats", str(a.repeats)]
    txt = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout
    return json.loads([ln for ln in txt.splitlines() if ln.startswith("RESULT ")][-1][7:])


def spread(v):
    v = np.asarray(v, dtype=float)
    return dict(median=round(float(np.median(v)), 3), min=round(float(v.min()), 3), max=round(float(v.max()), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--region_kb", type=int, nargs="+", default=[100, 500])
    ap.add_argument("--bam_dir", default=None)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--threads", type=int, nargs="+", default=[16, 2])
    ap.add_argument("--parent_root", default=None)
    ap.add_argument("--variants", action="store_true")
    ap.add_argument("--stream_file", default=None, help="--variants: the bytes to code (default: the inflated mix of the first region, host path)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deflate_bench.jsonl"))
    ap.add_argument("--worker", action="store_true")
    for name in ("root", "deflate", "tumor", "normal"):
        ap.add_argument("--" + name, default=None)
    ap.add_argument("--host_threads", type=int, default=16)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))

    def emit(rec):
        print(json.dumps(rec))
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")

    bam_dir = a.bam_dir or tempfile.mkdtemp()
    bams = {}
    for kb in a.region_kb:
        for kind, seed in (("t", 1), ("n", 2)):
            bams[kind, kb] = os.path.join(bam_dir, "contam_bench_%s_%d.bam" % (kind, kb))
            if not os.path.exists(bams[kind, kb]):
                from cal_af_bench import write_synthetic_bam
                write_synthetic_bam(bams[kind, kb], kb * 1000, 30, seed=seed)
    if a.variants:
        import contamutil as cu
        from clairs_to_amd.gen_contaminated_bam import mix_bams
        tmp = tempfile.mkdtemp()
        stream_file = a.stream_file
        kb = a.region_kb[0]
        if stream_file is None:
            mix_bams(bams["t", kb], bams["n", kb], os.path.join(tmp, "mix.bam"), 700, 300, where="host", host_threads=a.threads[0])
            stream_file = os.path.join(tmp, "stream.bin")
            with open(stream_file, "wb") as f:
                f.write(cu.inflated(os.path.join(tmp, "mix.bam"))[0])
        for seg, probes in VARIANTS:
            exe = os.path.join(tmp, "ratio_%d_%s" % (seg, probes.replace(",", "_")))
            subprocess.run(["g++", "-O2", "-std=c++17", "-DCTO_DEFLATE_SEG=%d" % seg, "-DCTO_DEFLATE_PROBES=" + probes,
                            os.path.join(ROOT, "tools", "deflate_ratio.cpp"), "-o", exe], check=True)
            n_in, n_out, blocks, stored, fixed, dyn = (int(x) for x in subprocess.run([exe, stream_file], check=True, capture_output=True, text=True).stdout.split())
            emit(dict(tool="deflate_bench", what="variant", region_kb=kb, segment=seg, probes=probes, in_bytes=n_in, out_bytes=n_out,
                      ratio=round(n_out / n_in, 4), blocks=blocks, types=[stored, fixed, dyn]))
        return
    for kb in a.region_kb:
        t, n = bams["t", kb], bams["n", kb]
        sized = False
        for threads in a.threads:
            runs = {}
            todo = [("zlib", ROOT), ("device", ROOT), ("host", ROOT)] + ([("parent", a.parent_root)] if a.parent_root else [])
            for deflate, root in todo:
                r = runs[deflate] = run_worker(root, deflate, t, n, threads, a)
                wc = [x["ms_write"] + x["ms_copy"] for x in r["reps"]]
                emit(dict(tool="deflate_bench", what="time", region_kb=kb, deflate=deflate, where="device", host_threads=threads, warmup=a.warmup,
                          repeats=a.repeats, ms_write_plus_copy=spread(wc), ms_write_plus_copy_all=[round(x, 3) for x in wc],
                          ms_write=spread([x["ms_write"] for x in r["reps"]]), ms_copy=spread([x["ms_copy"] for x in r["reps"]]),
                          ms_deflate_kernels=spread([x["ms_deflate_kernels"] for x in r["reps"]]), wall_ms=spread([x["wall_ms"] for x in r["reps"]]),
                          ms_mix_kernels=spread([x["ms_kernels"] for x in r["reps"]]), fallback_chunks=max(x["fallback"] for x in r["reps"]),
                          out_bytes=r["out_bytes"], stream_bytes=r["stream_bytes"], block_types=r["types"]))
            if not sized:                                   # zlib on the same blocks, once per size
                import contamutil as cu
                sized = True
                stream = cu.inflated(runs["device"]["out"])[0]
                sizes = {}
                for level in (1, 6):
                    total = 28
                    for at in range(0, len(stream), 0xff00):
                        co = zlib.compressobj(level, zlib.DEFLATED, -15)
                        total += len(co.compress(stream[at:at + 0xff00]) + co.flush()) + 26
                    sizes[level] = total
                assert sizes[6] == runs["zlib"]["out_bytes"], "zlib level 6 in Python and in the writer differ"
                emit(dict(tool="deflate_bench", what="ratio", region_kb=kb, stream_bytes=len(stream), device_coder_bytes=runs["device"]["out_bytes"],
                          host_coder_bytes=runs["host"]["out_bytes"], zlib1_bytes=sizes[1], zlib6_bytes=sizes[6],
                          device_ratio=round(runs["device"]["out_bytes"] / len(stream), 4), zlib1_ratio=round(sizes[1] / len(stream), 4),
                          zlib6_ratio=round(sizes[6] / len(stream), 4), block_types=runs["device"]["types"]))


if __name__ == "__main__":
    main()
