#!/usr/bin/env python3
"""The reference's gen_contaminated_bam (src/gen_contaminated_bam.py), run from /root/reference under --dry_run 1 (needs the reference
checkout; no BAM is opened and no command is run) -> contam_dry_run.json.gz.

Stored, data only: per argument set the argv, and the lines the reference printed that carry values - the coverage line, the subsample
proportions, the warning of the "use all normal" branch, the two merge lines - in the order it printed them; its "Calculating coverage"
and "Will run the following commands" lines and the command lines themselves are left out.  The option table of its parser.
The sets cover: both coverages given, one given, none given (a coverage not given is 1 under --dry_run); purities 0.2 / 0.5 / 0.8 / 1.0
and none; contamination above the normal's coverage; ratios that round to "1.000" and "0.000"; with and without --ctg_name.
Usage: python tests/golden/gen_contam.py"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, HERE)

import gen_cli  # noqa: E402

CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
sys.argv = ["gen_contaminated_bam"] + sys.argv[2:]
from src.gen_contaminated_bam import main
main()
"""

KEPT = ("[INFO] Normal/Tumor BAM coverage:", "[INFO] Normal/Tumor subsample proportion:", "[WARNING] Contaim coverage",
        "[INFO] Merging normal BAM into tumor BAM", "[INFO] Finishing merging, output file:")


def case(name, normal=None, tumor=None, purity=None, ctg=None, extra=()):
    argv = ["--normal_bam_fn", "n.bam", "--tumor_bam_fn", "t.bam", "--output_dir", "out_" + name, "--dry_run", "1"]
    if normal is not None:
        argv += ["--normal_bam_coverage", str(normal)]
    if tumor is not None:
        argv += ["--tumor_bam_coverage", str(tumor)]
    if purity is not None:
        argv += ["--tumor_purity", str(purity)]
    if ctg is not None:
        argv += ["--ctg_name", ctg]
    return dict(name=name, argv=argv + list(extra))


CASES = [case("both_p02", 30, 60, 0.2), case("both_p05", 30, 60, 0.5), case("both_p08", 30, 60, 0.8), case("both_p10", 30, 60, 1.0),
         case("both_none", 30, 60), case("both_p05_ctg", 45.5, 75.25, 0.5, ctg="chr20"),
         case("normal_only_p05", normal=30, purity=0.5), case("tumor_only_p08", tumor=60, purity=0.8), case("tumor_only_p02", tumor=60, purity=0.2),
         case("none_p05", purity=0.5), case("none_p02_ctg", purity=0.2, ctg="chr1"), case("none_none"),
         case("warn_p02", 10, 80, 0.2), case("warn_p05_ctg", 20.5, 90, 0.5, ctg="chrX"),
         case("round_one", 30.0001, 60, 0.5), case("round_zero", 90000, 60, 0.9999), case("thirds", 33, 77, 0.3333),
         case("ctg_none_string", 30, 60, 0.5, ctg="None"), case("tools_named", 30, 60, 0.8, extra=("--samtools", "/x/samtools", "--mosdepth", "/x/mosdepth",
                                                                                               "--samtools_threads", "4")),
         case("equal_cov", 12, 60, 0.8)]


def main():
    assert os.path.isdir(REF)
    tmp = tempfile.mkdtemp(prefix="gen_contam_")
    out = []
    for c in CASES:
        p = subprocess.run([sys.executable, "-W", "ignore", "-c", CHILD, REF] + c["argv"], cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert p.returncode == 0, (c, p.stderr[-3000:])
        lines = [ln for ln in p.stdout.split("\n") if ln.startswith(KEPT)]
        print(c["name"], lines, flush=True)
        out.append(dict(name=c["name"], argv=c["argv"], lines=lines))
    by = {o["name"]: o["lines"] for o in out}
    assert len(by["both_none"]) == 1 and len(by["both_p05"]) == 4 and len(by["warn_p02"]) == 5
    assert any("1.000/" in ln for ln in by["round_one"]) and any(": 0.000/" in ln for ln in by["round_zero"])
    assert by["none_p05"][0].endswith(": 1/1")
    parser = json.loads(subprocess.run([sys.executable, "-c", gen_cli.PARSER_PROBE % REF, "src.gen_contaminated_bam"], stdout=subprocess.PIPE,
                                       check=True, cwd=tmp).stdout.decode().strip().split("\n")[-1])
    assert len(parser) == 13, parser
    gen_cli.dump_json_gz("contam_dry_run.json.gz", dict(cases=out, parser=parser))
    shutil.rmtree(tmp, ignore_errors=True)
    print("wrote contam_dry_run.json.gz", os.path.getsize(os.path.join(HERE, "contam_dry_run.json.gz")), "bytes")


if __name__ == "__main__":
    main()
