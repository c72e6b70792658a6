#!/usr/bin/env python3
"""The reference's cal_af (src/cal_af_distribution.py:137-210), run from /root/reference on the case of tests/calafutil.py (needs the
reference checkout and gzip) -> cal_af.json.gz.  The reference starts `samtools mpileup ... -r ctg:p-p` once per truth variant; there is
no samtools here, so --samtools points at a throw-away stand-in that checks the command line it is given (mpileup, --min-MQ 20,
--min-BQ 0, --excl-flags 2316, the BAM) and prints the row calafutil.mpileup_row() states for that position - seven columns with
--output-extra HP, six without, `^` / `$` / `>` / `<` included, nothing where no read covers.  What the reference makes of those rows,
of the two VCFs and of its options is what the fixture pins; that the rows are what samtools prints is not pinned (csrc/aftally.hip).

Stored, data only: the seed of the case and a SHA-256 of its reads; both VCF texts; the rows served; per configuration the Namespace,
the reference's output file, its returned dict (as [key, value] pairs, with and without --output_path) and what it printed; the option
table of the reference's parser.  Configurations: --ctg_name chrB and none, each with and without --phase_output, all with
--truth_filter_tag PASS; and chrB without a filter tag.  The truth file is gzip-compressed in the runs without --ctg_name.
Usage: python tests/golden/gen_cal_af.py"""
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import calafutil  # noqa: E402
import gen_cli  # noqa: E402

STAND_IN = r'''#!%s
import json, os, sys
a = sys.argv[1:]
rows = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "rows.json")))
ok = a[0] == "mpileup" and a[a.index("--min-MQ") + 1] == "20" and a[a.index("--min-BQ") + 1] == "0" and a[a.index("--excl-flags") + 1] == "2316"
hp = "--output-extra" in a and a[a.index("--output-extra") + 1] == "HP"
rest = [x for i, x in enumerate(a[1:], 1) if not x.startswith("-") and a[i - 1] not in ("--min-MQ", "--min-BQ", "--excl-flags", "--output-extra", "-r")]
region = a[a.index("-r") + 1]
ctg, span = region.rsplit(":", 1)
lo, hi = span.split("-")
if not ok or rest != ["t.bam"] or lo != hi:
    sys.exit("stand-in: unexpected command line %%r" %% (a,))
sys.stdout.write(rows["%%s:%%s:%%d" %% (ctg, lo, hp)])
'''

CHILD = r"""
import argparse, json, sys
sys.path.insert(0, sys.argv[1])
from src.cal_af_distribution import cal_af
r = cal_af(argparse.Namespace(**json.loads(sys.argv[2])))
print("SEEN " + json.dumps(None if r is None else [[k, v] for k, v in r.items()]))
"""

CONFIGS = [dict(name="chrB_hp", ctg_name="chrB", phase_output=True, truth_filter_tag="PASS", gz=False),
           dict(name="chrB_nohp", ctg_name="chrB", phase_output=False, truth_filter_tag="PASS", gz=False),
           dict(name="all_hp", ctg_name=None, phase_output=True, truth_filter_tag="PASS", gz=True),
           dict(name="all_nohp", ctg_name=None, phase_output=False, truth_filter_tag="PASS", gz=True),
           dict(name="chrB_hp_any_filter", ctg_name="chrB", phase_output=True, truth_filter_tag=None, gz=False)]


def run_ref(tmp, ns):
    p = subprocess.run([sys.executable, "-W", "ignore", "-c", CHILD, REF, json.dumps(ns)], cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, (ns, p.stderr[-3000:])
    lines = p.stdout.split("\n")
    seen = [ln for ln in lines if ln.startswith("SEEN ")][-1]
    return json.loads(seen[5:]), "".join(ln + "\n" for ln in lines if ln and not ln.startswith("SEEN "))


def main():
    assert os.path.isdir(REF)
    tmp = tempfile.mkdtemp(prefix="gen_cal_af_")
    c = calafutil.case()
    truth, inp = calafutil.vcf_texts()
    open(os.path.join(tmp, "truth.vcf"), "w").write(truth)
    with gzip.open(os.path.join(tmp, "truth.vcf.gz"), "wt") as f:
        f.write(truth)
    open(os.path.join(tmp, "input.vcf"), "w").write(inp)
    # every position either VCF names, with and without the HP column
    rows = {}
    for text in (truth, inp):
        for ln in text.split("\n"):
            if ln and ln[0] != "#":
                ctg, pos = ln.split("\t")[:2]
                for hp in (0, 1):
                    rows["%s:%s:%d" % (ctg, pos, hp)] = calafutil.mpileup_row(c["entered"][ctg], ctg, int(pos), bool(hp))
    json.dump(rows, open(os.path.join(tmp, "rows.json"), "w"))
    tool = os.path.join(tmp, "samtools")
    open(tool, "w").write(STAND_IN % sys.executable)
    os.chmod(tool, 0o755)
    out = []
    for cf in CONFIGS:
        ns = dict(tumor_bam_fn="t.bam", input_vcf_fn="input.vcf", truth_vcf_fn="truth.vcf.gz" if cf["gz"] else "truth.vcf", input_filter_tag=None,
                  truth_filter_tag=cf["truth_filter_tag"], ctg_name=cf["ctg_name"], output_path="out.txt", threads=4, phase_output=cf["phase_output"],
                  samtools=tool, min_mq=20, min_bq=0, min_bq_cut=0)
        none, printed = run_ref(tmp, ns)
        assert none is None
        text = open(os.path.join(tmp, "out.txt")).read()
        os.remove(os.path.join(tmp, "out.txt"))
        pairs, printed2 = run_ref(tmp, dict(ns, output_path=None))
        n4 = sum(len(ln.split(" ")) == 4 for ln in text.split("\n") if ln)
        n10 = sum(len(ln.split(" ")) == 10 for ln in text.split("\n") if ln)
        print(cf["name"], "rows", n4, "+", n10, "dict", len(pairs), repr(printed), flush=True)
        assert n4 >= 5 and n10 >= 50 and len(pairs) == n4 + n10 and printed == printed2
        first10 = next(i for i, ln in enumerate(text.split("\n")) if len(ln.split(" ")) == 10)
        assert first10 == n4                                      # the input-VCF rows come first
        out.append(dict(name=cf["name"], namespace=dict(ns, samtools="samtools"), gz=cf["gz"], output=text, returned=pairs, printed=printed))
    by = {o["name"]: o for o in out}
    assert by["chrB_hp"]["output"] != by["chrB_nohp"]["output"] and len(by["chrB_hp_any_filter"]["output"]) > len(by["chrB_hp"]["output"])
    assert any(ln.split(" ")[4:7] != ["0", "0", "0"] for ln in by["all_hp"]["output"].split("\n") if len(ln.split(" ")) == 10)
    assert " 10 2\n" in by["all_hp"]["output"]                     # round(0.25 * 10) == 2
    parser = json.loads(subprocess.run([sys.executable, "-c", gen_cli.PARSER_PROBE % REF, "src.cal_af_distribution"], stdout=subprocess.PIPE, check=True,
                                       cwd=tmp).stdout.decode().strip().split("\n")[-1])
    assert len(parser) == 13, parser
    gen_cli.dump_json_gz("cal_af.json.gz", dict(seed=calafutil.SEED, reads_sha256=calafutil.reads_digest(c["reads"]), n_reads=len(c["reads"]), truth_vcf=truth,
                                                input_vcf=inp, rows=rows, configs=out, parser=parser))
    shutil.rmtree(tmp, ignore_errors=True)
    size = os.path.getsize(os.path.join(HERE, "cal_af.json.gz"))
    print("wrote cal_af.json.gz", size, "bytes")
    assert size < os.path.getsize(os.path.join(HERE, "region2k.json.gz"))


if __name__ == "__main__":
    main()
