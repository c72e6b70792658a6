"""Pin-on-arrival for the allele counter ("parity unpinned against alleleCounter").
    python tools/pin_allelecounter.py [--allelecounter alleleCounter] [--keep DIR] [--self-check]
Needs a real `alleleCounter` (htslib; none in the build image, none on the GPU machine).  On the BAM the test-suite generates
(tests/allelecountutil.py: every CIGAR operation, loci inside D and N, missing qualities, IUPAC bases, the flag masks, mate pairs that
agree / disagree / are deleted at the locus, three reads of one name, a locus deeper than 2048) it runs
    alleleCounter -b BAM -l LOCI -o OUT -m M -q Q -f f -F F --dense-snps
for every parameter set of the tests and compares the table, byte for byte, with `python -m clairs_to_amd allele_counter --where host`.
Three rules rest on htslib's behaviour as known, not on a run (the pile-up iterator's own 1796 mask, the query index inside D / N, 0xff
qualities): a difference at flag512 / flag1024, at the loci inside `dn`, or at `noqual` names which one.
--self-check runs the comparison half against our own output (device against host when a GPU is present, else host against host).
Exit code = verdict: 0 all equal, 1 a difference (the first rows of it printed), 2 cannot pin here (no alleleCounter)."""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)


def first_difference(a, b):
    la, lb = a.split("\n"), b.split("\n")
    for i in range(max(len(la), len(lb))):
        x, y = (la[i] if i < len(la) else "<end>"), (lb[i] if i < len(lb) else "<end>")
        if x != y:
            return "row %d: %r / %r" % (i, x, y)
    return None


def ours(bam, loci_fn, out_fn, params, where):
    from clairs_to_amd.allele_counter import main as ac_main
    bq, mq, f, F = params
    ac_main(["-b", bam, "-l", loci_fn, "-o", out_fn, "-m", str(bq), "-q", str(mq), "-f", str(f), "-F", str(F), "-d", "--where", where])
    return open(out_fn).read()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--allelecounter", default="alleleCounter")
    ap.add_argument("--keep", default=None, help="leave the loci file and the tables in this directory")
    ap.add_argument("--self-check", action="store_true")
    a = ap.parse_args()
    if not a.self_check and shutil.which(a.allelecounter) is None:
        print("pin_allelecounter: `%s` not found: cannot pin here" % a.allelecounter)
        sys.exit(2)
    from allelecountutil import PARAMS, case, loci_file_lines
    tmp = a.keep or tempfile.mkdtemp(prefix="pin_allelecounter_")
    os.makedirs(tmp, exist_ok=True)
    loci_fn = os.path.join(tmp, "loci.txt")
    open(loci_fn, "w").write("\n".join(loci_file_lines()) + "\n")
    bam = case()["bam"]
    other = "host"
    if a.self_check:
        import torch
        other = "device" if torch.cuda.is_available() else "host"
    bad = 0
    for name, params in sorted(PARAMS.items()):
        mine = ours(bam, loci_fn, os.path.join(tmp, "ours_%s.txt" % name), params, "host")
        theirs_fn = os.path.join(tmp, "theirs_%s.txt" % name)
        if a.self_check:
            theirs = ours(bam, loci_fn, theirs_fn, params, other)
        else:
            bq, mq, f, F = params
            cmd = [a.allelecounter, "-b", bam, "-l", loci_fn, "-o", theirs_fn, "-m", str(bq), "-q", str(mq), "-f", str(f), "-F", str(F), "--dense-snps"]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            if p.returncode != 0:
                sys.exit("pin_allelecounter: %s failed: %s" % (" ".join(cmd), p.stderr.decode()[-400:]))
            theirs = open(theirs_fn).read()
        d = first_difference(mine, theirs)
        print("%-9s -m %d -q %d -f %d -F %d: %s" % ((name,) + tuple(params) + ("equal" if d is None else "DIFFERENT - " + d,)))
        bad += d is not None
    print("pin_allelecounter: %d parameter sets, %d differ (%s)" % (len(PARAMS), bad, "our %s path" % other if a.self_check else a.allelecounter))
    if not a.keep:
        shutil.rmtree(tmp, ignore_errors=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
