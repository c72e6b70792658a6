"""The reference's src/gen_contaminated_bam.py: a tumour BAM of a chosen purity, made by mixing a share of a normal BAM into a share of the
tumour BAM - what the reference's benchmarking BAMs come from.  The reference starts `mosdepth -n -x` (twice), `samtools view -s` (twice),
`samtools merge` and `samtools index` for it; here cto_bam_coverage and cto_bam_mix (csrc/contam.hip: the device path; csrc/bam.cpp: the host
path) do the work, subsample and merge in one pass.  No mosdepth or samtools is involved.  PARITY UNPINNED against those programs: the rules
are this package's own (csrc/contam.hip lists them).

    python -m clairs_to_amd gen_contaminated_bam --normal_bam_fn N.bam --tumor_bam_fn T.bam --output_dir DIR --tumor_purity 0.5
        [--normal_bam_coverage X] [--tumor_bam_coverage Y] [--ctg_name CTG] [--cal_output_bam_coverage 1] [--seed 0] [--where device|host]
        [--deflate zlib|device|host]

--deflate chooses the coder of the output's BGZF blocks: zlib level 6 on the host threads (the default), csrc/deflate.hip on the device
(with --where device the merged stream never comes down, only its compressed blocks do), or that coder's host restatement.  The last
two write the same bytes; the records, the block cuts and the index rules are those of zlib's file.

The options are the reference parser's.  The lines that carry values are printed as the reference prints them; its "Will run the following
commands" lines are not, since no command is run.  A coverage that is not given is computed and written where the reference expects
mosdepth's summary (<output_dir>/tmp/raw_{normal,tumor}.cov.mosdepth.summary.txt, <output_dir>/cov.cov.mosdepth.summary.txt), then read back
from that file as the reference reads it.  The reference's two intermediate BAMs (tmp/tumor_rest.bam, tmp/normal_subsample.bam) are not
written.  --remove_intermediate_dir removes <output_dir>/tmp; in the reference that flag raises an AttributeError (os.path.exist), which
is not reproduced."""
import ctypes as C
import os
import shutil
import struct
import sys
from argparse import ArgumentParser

from ._cli import add_ignored, str2bool, str_none

COV_SUFFIX = ".cov.mosdepth.summary.txt"
DEFLATE_MODES = ("zlib", "device", "host")          # cto_bam_mix_ex's deflate: 0, 1, 2
MAX_THREADS = 16


def _default_where():
    import torch
    return "device" if torch.cuda.is_available() else "host"


def _where_args(where):
    if where not in ("device", "host"):
        raise ValueError("where must be 'device' or 'host'")
    if where == "host":
        return 0, None
    from ._lib import current_stream_ptr
    return 1, C.c_void_p(current_stream_ptr())


def _path(p):
    return str(p).encode() if p else None


def _stats_into(stats, st):
    if stats is None:
        return
    for name, kind in st._fields_:
        v = getattr(st, name)
        if name in ("candidates", "kept"):
            v = [int(v[0]), int(v[1])]
            old = stats.get(name, [0, 0])
            stats[name] = [old[0] + v[0], old[1] + v[1]]
        else:
            stats[name] = stats.get(name, 0) + v


# ------------------------------------------------------------------------------------------ the engine
def reference_list(bam):
    """[(name, length)] of the BAM's header, in header order"""
    from .phase_tumor import BgzfReader
    rd = BgzfReader(str(bam))
    try:
        head = rd.read(8)
        if head[:4] != b"BAM\1":
            raise ValueError("gen_contaminated_bam: %s is not a BAM file" % bam)
        rd.read(struct.unpack_from("<i", head, 4)[0])
        out = []
        for _ in range(struct.unpack("<i", rd.read(4))[0]):
            name = rd.read(struct.unpack("<i", rd.read(4))[0])
            out.append((name.rstrip(b"\0").decode(), struct.unpack("<i", rd.read(4))[0]))
        return out
    finally:
        rd.close()


def bam_coverage(bam, ctg=None, where="device", bai=None, host_threads=0, stats=None):
    """cto_bam_coverage: `mosdepth -n -x` of one contig, or of every contig in header order when ctg is None ->
    [dict(chrom, length, bases, min, max)].  where: "device" (HIP kernels on the current stream) or "host".  stats: a dict that receives
    the call's cto_contam_stats."""
    from ._lib import ContamStats, CovRow, check, lib
    w, stream = _where_args(where)
    refs = reference_list(bam)
    rows = (CovRow * max(len(refs), 1))()
    st = ContamStats()
    n = check(lib.cto_bam_coverage(_path(bam), _path(bai), ctg.encode() if ctg is not None else None, w, int(host_threads), stream, rows, len(rows),
                                   C.byref(st)))
    _stats_into(stats, st)
    return [dict(chrom=refs[r.tid][0], length=int(r.length), bases=int(r.bases), min=int(r.min), max=int(r.max)) for r in rows[:n]]


def mix_bams(tumor_bam, normal_bam, out_bam, m_tumor, m_normal, seed=0, ctg=None, where="device", tumor_bai=None, normal_bai=None,
             host_threads=0, stats=None, deflate="zlib", deflate_stats=None):
    """cto_bam_mix: `samtools view -s SEED.ddd` of both BAMs and `samtools merge` + `samtools index` of what is kept, in one pass, into
    out_bam and out_bam + '.bai'.  m_tumor / m_normal: the proportions in thousandths, 0 .. 1000 (the reference's "%.3f" strings); 1000
    keeps every record, as -s 1.000 does, and 0 keeps none - unlike samtools, where -s 0.000 switches subsampling off and keeps all.
    ctg: one contig, or None for every contig in header order.  deflate: the coder of the output's blocks, "zlib" (level 6), "device"
    (csrc/deflate.hip) or "host" (its host restatement; the same bytes as "device"); deflate_stats: a dict that receives its
    cto_deflate_stats.  -> dict(candidates [tumour, normal], kept [tumour, normal])"""
    from ._lib import ContamStats, DeflateStats, check, lib
    w, stream = _where_args(where)
    if deflate not in DEFLATE_MODES:
        raise ValueError("deflate must be one of %s" % ", ".join(DEFLATE_MODES))
    st, dst = ContamStats(), DeflateStats()
    if deflate == "device" and stream is None:
        from ._lib import current_stream_ptr
        stream = C.c_void_p(current_stream_ptr())
    check(lib.cto_bam_mix_ex(_path(tumor_bam), _path(tumor_bai), _path(normal_bam), _path(normal_bai), ctg.encode() if ctg is not None else None,
                             int(m_tumor), int(m_normal), int(seed) & 0xffffffff, _path(out_bam), w, int(host_threads), stream, C.byref(st),
                             DEFLATE_MODES.index(deflate), C.byref(dst)))
    _stats_into(stats, st)
    _stats_into(deflate_stats, dst)
    return dict(candidates=[int(st.candidates[0]), int(st.candidates[1])], kept=[int(st.kept[0]), int(st.kept[1])])


def subsample_keys(names, seed=0, m=1000):
    """rule b on a list of read names (str or bytes) -> (k & 0xffffff as uint32 array, keep as bool array)"""
    import numpy as np
    from ._lib import check, lib
    raw = [n if isinstance(n, bytes) else n.encode() for n in names]
    off = np.zeros(len(raw) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in raw])
    buf = np.frombuffer(b"".join(raw) + b"\0", dtype=np.uint8)
    k24 = np.zeros(len(raw), dtype=np.uint32)
    keep = np.zeros(len(raw), dtype=np.uint8)
    check(lib.cto_subsample_keys(buf.ctypes.data, off.ctypes.data, len(raw), int(seed) & 0xffffffff, int(m), k24.ctypes.data, keep.ctypes.data))
    return k24, keep.astype(bool)


# ------------------------------------------------------------------------------------------ mosdepth's summary
def write_summary(fn, rows):
    """chrom length bases mean min max, one row per contig and the total row"""
    def line(name, length, bases, lo, hi):
        return "%s\t%d\t%d\t%s\t%d\t%d\n" % (name, length, bases, "%.2f" % (bases / length if length else 0.0), lo, hi)
    with open(fn, "w") as f:
        f.write("chrom\tlength\tbases\tmean\tmin\tmax\n")
        for r in rows:
            f.write(line(r["chrom"], r["length"], r["bases"], r["min"], r["max"]))
        f.write(line("total", sum(r["length"] for r in rows), sum(r["bases"] for r in rows), min([r["min"] for r in rows] or [0]),
                     max([r["max"] for r in rows] or [0])))


def read_summary(fn, ctg):
    """the coverage as the reference takes it from the file: the last row's mean, or the contig's"""
    with open(fn) as f:
        rows = f.readlines()
    if ctg is None:
        return float(rows[-1].split()[3])
    mine = [row for row in rows if row.split()[0] == ctg]
    if not mine:
        sys.exit("[ERROR] no contig coverage found for contig {}".format(ctg))
    return float(mine[0].split()[3])


def coverage_of(args, bam_fn, is_tumor, where, output_prefix=None):
    if args.dry_run:
        return 1
    if output_prefix is None:
        output_prefix = os.path.join(args.output_dir, "tmp", "raw_{}".format("tumor" if is_tumor else "normal"))
    fn = output_prefix + COV_SUFFIX
    write_summary(fn, bam_coverage(bam_fn, args.ctg_name, where=where, host_threads=args.samtools_threads))
    return read_summary(fn, args.ctg_name)


# ------------------------------------------------------------------------------------------ the step
def gen_contaminated_bam(args):
    where = args.where or ("host" if args.dry_run else _default_where())
    output_dir, purity = args.output_dir, args.tumor_purity
    if not args.dry_run:
        os.makedirs(os.path.join(output_dir, "tmp"), exist_ok=True)
    normal_cov = args.normal_bam_coverage if args.normal_bam_coverage else coverage_of(args, args.normal_bam_fn, False, where)
    tumor_cov = args.tumor_bam_coverage if args.tumor_bam_coverage else coverage_of(args, args.tumor_bam_fn, True, where)
    print("[INFO] Normal/Tumor BAM coverage: {}/{}".format(normal_cov, tumor_cov))
    if purity is None:
        return None
    contam_cov = tumor_cov * (1 - purity)
    rest_cov = tumor_cov - contam_cov
    if contam_cov > float(normal_cov):
        print("[WARNING] Contaim coverage is higher than normal, use all normal BAM!")
        normal_pro, m_normal = "1.00", 1000
    else:
        normal_pro = "%.3f" % (contam_cov / float(normal_cov))
        m_normal = int(round(float(normal_pro) * 1000))
    tumor_pro = "%.3f" % (rest_cov / float(tumor_cov))
    m_tumor = int(round(float(tumor_pro) * 1000))
    print("[INFO] Normal/Tumor subsample proportion: {}/{}".format(normal_pro, tumor_pro))
    out_bam = os.path.join(output_dir, "tumor_purity_{}.bam".format(purity))
    print("[INFO] Merging normal BAM into tumor BAM as contamination...")
    res = None
    if not args.dry_run:
        for name, v in (("normal", m_normal), ("tumor", m_tumor)):
            if not 0 <= v <= 1000:
                sys.exit("gen_contaminated_bam: the {} subsample proportion {} is outside 0 .. 1".format(name, v / 1000.0))
        print("[INFO] BGZF deflate of the output: {}".format(args.deflate))
        res = mix_bams(args.tumor_bam_fn, args.normal_bam_fn, out_bam, m_tumor, m_normal, seed=args.seed, ctg=args.ctg_name, where=where,
                       host_threads=args.samtools_threads, deflate=args.deflate)
        if args.cal_output_bam_coverage:
            coverage_of(args, out_bam, True, where, os.path.join(output_dir, "cov"))
        if args.remove_intermediate_dir:
            shutil.rmtree(os.path.join(output_dir, "tmp"), ignore_errors=True)
    print("[INFO] Finishing merging, output file: {}".format(out_bam))
    return res


def build_parser():
    ap = ArgumentParser(prog="gen_contaminated_bam", description="Generate contaminated BAM for benchmarking")
    ap.add_argument("--normal_bam_fn", type=str, default=None, help="Sorted normal BAM file input")
    ap.add_argument("--tumor_bam_fn", type=str, default=None, help="Sorted tumor BAM file input")
    ap.add_argument("--normal_bam_coverage", type=float, default=None, help="Normal BAM coverage; computed when absent")
    ap.add_argument("--tumor_bam_coverage", type=float, default=None, help="Tumor BAM coverage; computed when absent")
    ap.add_argument("--output_dir", type=str, default=None, help="Output directory: tumor_purity_<purity>.bam and its .bai")
    ap.add_argument("--samtools_threads", type=int, default=32, help="Host threads (deflate of the output), at most %d" % MAX_THREADS)
    ap.add_argument("--tumor_purity", type=float, default=None, help="Tumor purity")
    ap.add_argument("--ctg_name", type=str_none, default=None, help="The name of sequence to be processed")
    ap.add_argument("--dry_run", type=str2bool, default=0, help="EXPERIMENTAL: Only print the synthetic log, debug only")
    ap.add_argument("--cal_output_bam_coverage", type=str2bool, default=0, help="EXPERIMENTAL: calculate the coverage of the output BAM")
    ap.add_argument("--remove_intermediate_dir", action="store_true", help="Remove intermediate directory. Default: False")
    ap.add_argument("--where", type=str, default=None, choices=("device", "host"), help="Where the BAMs are read, default: device when there is one")
    ap.add_argument("--deflate", type=str, default="zlib", choices=DEFLATE_MODES,
                    help="The coder of the output's BGZF blocks: zlib level 6, the device coder, or its host restatement, default: %(default)s")
    ap.add_argument("--seed", type=int, default=0, help="The subsampling seed: the integer part of the reference's `-s 0.ddd`, default: %(default)d")
    add_ignored(ap, samtools="str", mosdepth="str")
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(sys.argv[1:] if argv is None else argv)
    for name in ("normal_bam_fn", "tumor_bam_fn", "output_dir"):
        if getattr(args, name) is None and not args.dry_run:
            sys.exit("gen_contaminated_bam: --%s is required" % name)
    args.samtools_threads = max(1, min(int(args.samtools_threads), MAX_THREADS))
    from ._lib import CtoError
    try:
        gen_contaminated_bam(args)
    except (CtoError, ValueError) as e:
        sys.exit("gen_contaminated_bam: %s" % e)


if __name__ == "__main__":
    main()
