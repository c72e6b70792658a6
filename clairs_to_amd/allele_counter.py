"""alleleCounter without htslib: the per-locus A / C / G / T counts of a BAM, the first command of the reference's Verdict step
(src/cna_germline_tagging.py:56-71 runs `alleleCounter -b BAM -l LOCI -o OUT -m 20 -q 20 -f 0 -F 2316 --dense-snps` per contig).
The counting is cto_allele_counts (csrc/allelecount.hip: the rules, the device path; csrc/bam.cpp: the host path); this module reads
the loci file, sorts it as the program does, writes the program's table.  PARITY UNPINNED against alleleCounter.

    python -m clairs_to_amd allele_counter -b BAM -l LOCI -o OUT [-m 20] [-q 35] [-f 3] [-F 3852] [-d] [--where device|host]
    python -m clairs_to_amd allele_counter -b BAM --contig_fn CONTIGS --loci_prefix P --output_prefix O ...       (an addition, see main)
"""
import argparse
import ctypes as C
import re
import sys

import numpy as np

HEADER = "#CHR\tPOS\tCount_A\tCount_C\tCount_G\tCount_T\tGood_depth\n"
MAJOR_CONTIGS = ["chr%s" % c for c in list(range(1, 23)) + ["X"]]        # src/cna_germline_tagging.py:41

_NUMERIC = re.compile(r"\s*([+-]?\d+)[ \t]+([+-]?\d+)")                  # sscanf "%d%*[ \t]%d"
_STRING = re.compile(r"\s*(\S+)[ \t]+([+-]?\d+)")                        # sscanf "%s%*[ \t]%d"


def _default_where():
    import torch
    return "device" if torch.cuda.is_available() else "host"


def count_alleles(bam, ctg, positions, min_bq=20, min_mq=35, req_flags=3, excl_flags=3852, where="device", bai=None, host_threads=0,
                  stats=None):
    """int32 [n, 4] counts of A, C, G, T at the 1-based `positions` (strictly ascending) of contig `ctg`; the defaults are
    alleleCounter's own.  where: "device" (HIP kernels on the current stream) or "host".  stats: a dict that receives the call's
    cto_allele_stats."""
    from ._lib import AlleleStats, check, lib
    if where not in ("device", "host"):
        raise ValueError("where must be 'device' or 'host'")
    loci = np.ascontiguousarray(positions, dtype=np.int32)
    counts = np.zeros((len(loci), 4), dtype=np.int32)
    st = AlleleStats()
    stream = None
    if where == "device":
        from ._lib import current_stream_ptr
        stream = C.c_void_p(current_stream_ptr())
    check(lib.cto_allele_counts(str(bam).encode(), str(bai).encode() if bai else None, ctg.encode(), loci.ctypes.data, len(loci),
                                int(min_bq), int(min_mq), int(req_flags), int(excl_flags), 1 if where == "device" else 0, int(host_threads),
                                stream, counts.ctypes.data, C.byref(st)))
    if stats is not None:
        for name, _ in AlleleStats._fields_:
            stats[name] = stats.get(name, 0) + getattr(st, name)
    return counts


def read_loci(path):
    """[(chr, pos)] of a loci file in file order: `chr<ws>pos`, further columns ignored; a chromosome written as a number comes back as
    that number's decimal string (alleleCounter.c:281-290)."""
    out = []
    with open(path) as f:
        for i, line in enumerate(f):
            m = _NUMERIC.match(line)
            if m:
                out.append((str(int(m.group(1))), int(m.group(2))))
                continue
            m = _STRING.match(line)
            if not m:
                sys.exit("allele_counter: cannot parse line %d of %s: %r" % (i + 1, path, line))
            out.append((m.group(1), int(m.group(2))))
    return out


def count_loci_file(bam, loci_fn, out_fn, where, stats=None, **kw):
    """One loci file -> one table, as the program writes it: rows sorted by strcmp(chr) then pos, one row per input line; a repeated
    locus prints its counts once and zeros for every repeat."""
    loci = read_loci(loci_fn)
    loci.sort(key=lambda cp: (cp[0].encode(), cp[1]))
    rows = np.zeros((len(loci), 4), dtype=np.int64)
    i = 0
    while i < len(loci):
        j = i
        while j < len(loci) and loci[j][0] == loci[i][0]:
            j += 1
        pos = np.array([p for _, p in loci[i:j]], dtype=np.int64)
        if pos.min() < 1 or pos.max() >= 2 ** 31:
            sys.exit("allele_counter: position out of range on %s in %s" % (loci[i][0], loci_fn))
        first = np.ones(len(pos), dtype=bool)
        first[1:] = pos[1:] != pos[:-1]
        rows[i:j][first] = count_alleles(bam, loci[i][0], pos[first], where=where, stats=stats, **kw)
        i = j
    with open(out_fn, "w") as f:
        f.write(HEADER)
        for (c, p), r in zip(loci, rows):
            f.write("%s\t%d\t%d\t%d\t%d\t%d\t%d\n" % (c, p, r[0], r[1], r[2], r[3], r.sum()))
    return len(loci)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="allele_counter", description="alleleCounter's options, verbatim, plus --where and a per-contig convenience")
    ap.add_argument("-l", "--loci-file")
    ap.add_argument("-b", "--hts-file", required=True)
    ap.add_argument("-o", "--output-file")
    ap.add_argument("-m", "--min-base-qual", type=int, default=20)
    ap.add_argument("-q", "--min-map-qual", type=int, default=35)
    ap.add_argument("-c", "--contig", default=None, help="accepted; the program parses it and never reads it")
    ap.add_argument("-d", "--dense-snps", action="store_true", help="accepted; both modes give the same counts")
    ap.add_argument("-f", "--required-flag", type=int, default=3)
    ap.add_argument("-F", "--filtered-flag", type=int, default=3852)
    ap.add_argument("-r", "--ref-file", default=None, help="accepted, unused (CRAM is not read)")
    ap.add_argument("-x", "--is-10x", action="store_true")
    ap.add_argument("--where", choices=("device", "host"), default=None, help="default: device when a GPU is present")
    ap.add_argument("--host_threads", type=int, default=0)
    # not the reference's argv: what tumor_allele_counter_command (src/cna_germline_tagging.py:56-71) does with GNU parallel, in one process
    ap.add_argument("--contig_fn", default=None, help="file of contig names; those among chr1..22, X are counted")
    ap.add_argument("--loci_prefix", default=None, help="loci file of a contig = <loci_prefix><contig>.txt")
    ap.add_argument("--output_prefix", default=None, help="table of a contig = <output_prefix><contig>.txt")
    a = ap.parse_args(argv)
    if a.is_10x:
        sys.exit("allele_counter: the 10x mode (-x) is not supported")
    if a.hts_file.lower().endswith(".cram"):
        sys.exit("allele_counter: CRAM input is not supported; give a BAM with its .bai")
    where = a.where or _default_where()
    kw = dict(min_bq=a.min_base_qual, min_mq=a.min_map_qual, req_flags=a.required_flag, excl_flags=a.filtered_flag, host_threads=a.host_threads)
    per_contig = (a.contig_fn, a.loci_prefix, a.output_prefix)
    if any(per_contig):
        if not all(per_contig) or a.loci_file or a.output_file:
            sys.exit("allele_counter: --contig_fn, --loci_prefix and --output_prefix go together, without -l / -o")
        with open(a.contig_fn) as f:
            contigs = [c.strip() for c in f if c.strip() in MAJOR_CONTIGS]
        for c in contigs:
            count_loci_file(a.hts_file, "%s%s.txt" % (a.loci_prefix, c), "%s%s.txt" % (a.output_prefix, c), where, **kw)
        return 0
    if not a.loci_file or not a.output_file:
        sys.exit("allele_counter: -l / --loci-file and -o / --output-file are required")
    count_loci_file(a.hts_file, a.loci_file, a.output_file, where, **kw)
    return 0


if __name__ == "__main__":
    main(sys.argv[1:])
