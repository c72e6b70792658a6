#!/usr/bin/env python3
"""The reference's select_hetero_snp_for_phasing (src/select_hetero_snp_for_phasing.py:40-103), run from /root/reference (needs the
reference checkout and gzip) on small pileup VCFs written here -> select_hetero.json.gz.

Stored, data only: the input VCF texts; per configuration the Namespace, whether the input went in gzip-compressed, the output file
<output_folder>/<ctg>.vcf and what the reference printed; the option table of the reference's parser.  The inputs hold, between them:
two contigs (read with --ctg_name), 0/1, 1/0, 0|1, 1|0, 1/1 and 0/0 genotypes, indel and multi-allelic rows, QUAL on both sides of
--min_qual (one exactly on it), QUAL ties for the --var_pct_full cut, a position given twice (the later row wins, the QUAL table keeps
the first place; once with the second QUAL below --min_qual), and header rows with trailing blanks.
Usage: python tests/golden/gen_select_hetero.py"""
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

import gen_cli  # noqa: E402

CHILD = r"""
import argparse, json, sys
sys.path.insert(0, sys.argv[1])
from src.select_hetero_snp_for_phasing import select_hetero_snp_for_phasing
select_hetero_snp_for_phasing(argparse.Namespace(**json.loads(sys.argv[2])))
"""

HEAD = ("##fileformat=VCFv4.2\n##FILTER=<ID=PASS,Description=\"All filters passed\">  \n##contig=<ID=chrA,length=100000>\n"
        "##contig=<ID=chrB,length=100000>\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
        "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n")


def row(ctg, pos, ref, alt, qual, gt, flt="PASS", af="0.4500"):
    return "%s\t%d\t.\t%s\t%s\t%s\t%s\t.\tGT:GQ:DP:AF\t%s:%s:30:%s\n" % (ctg, pos, ref, alt, qual, flt, gt, str(qual).split(".")[0], af)


def vcf_main():
    """two contigs; ties in QUAL; every genotype spelling; indels; a multi-allelic row; QUAL around min_qual 5"""
    rows = []
    quals = ["12.5", "8.0", "8.0", "30.25", "4.9999", "5.0", "8.0", "17", "3", "22.75", "8.0", "9.5", "40", "6.5", "2.5", "11", "8.0", "14", "19", "7"]
    gts = ["0/1", "1/0", "0|1", "1|0", "0/1", "0/1", "1/1", "0/1", "1|0", "0/0", "0/1", "./.", "0/1", "1/0", "0|1", "0/1", "0/1", "1|1", "0/1", "1/0"]
    for i, (q, gt) in enumerate(zip(quals, gts)):
        ref, alt = "ACGT"[i % 4], "CGTA"[i % 4]
        rows.append(row("chrA", 1000 + 137 * i, ref, alt, q, gt))
    rows.insert(4, row("chrA", 1500, "AT", "A", "33", "0/1"))              # deletion
    rows.insert(9, row("chrA", 2100, "G", "GTT", "28", "0/1"))             # insertion
    rows.insert(12, row("chrA", 2500, "C", "A,T", "21", "1/2"))            # multi-allelic
    rows.insert(13, row("chrA", 2600, "C", "A,T", "21", "0/1"))            # heterozygous, but ALT is three characters long
    for i in range(9):
        rows.append(row("chrB", 500 + 211 * i, "GTCA"[i % 4], "TCAG"[i % 4], ["6", "6", "15.5", "4", "6", "50", "6", "0.5", "9"][i],
                        ["0/1", "1|0", "0/1", "0/1", "1/0", "0|1", "1/1", "1/0", "0/1"][i]))
    return HEAD + "".join(rows)


def vcf_dup():
    """positions given twice: the later row replaces the earlier one; the QUAL table keeps the place of the first"""
    rows = [row("chrA", 100, "A", "C", "9", "0/1"), row("chrA", 200, "C", "G", "7", "0/1"), row("chrA", 300, "G", "T", "7", "1/0"),
            row("chrA", 100, "A", "G", "7", "0|1", af="0.3000"),          # replaces the row at 100; QUAL 9 -> 7, still first in the table
            row("chrA", 400, "T", "A", "7", "0/1"), row("chrA", 500, "A", "T", "20", "0/1"),
            row("chrA", 300, "G", "T", "1", "0/1", af="0.1000"),          # below min_qual: the earlier row at 300 stays, its QUAL becomes 1
            row("chrA", 600, "C", "T", "7", "1|0"), row("chrA", 700, "G", "A", "6.5", "0/1"), row("chrA", 50, "T", "C", "31", "0/1")]
    return HEAD + "".join(rows)


INPUTS = {"main": vcf_main, "dup": vcf_dup}
CONFIGS = [dict(name="chrA_pct0", vcf="main", ctg_name="chrA", var_pct_full=0.0, min_qual=5, gz=False),
           dict(name="chrB_pct0", vcf="main", ctg_name="chrB", var_pct_full=0.0, min_qual=5, gz=False),
           dict(name="chrA_pct01", vcf="main", ctg_name="chrA", var_pct_full=0.1, min_qual=5, gz=False),
           dict(name="chrA_pct05", vcf="main", ctg_name="chrA", var_pct_full=0.5, min_qual=5, gz=True),
           dict(name="chrB_pct05", vcf="main", ctg_name="chrB", var_pct_full=0.5, min_qual=5, gz=True),
           dict(name="chrA_minqual9", vcf="main", ctg_name="chrA", var_pct_full=0.1, min_qual=9, gz=False),
           dict(name="chrA_minqual0", vcf="main", ctg_name="chrA", var_pct_full=0.0, min_qual=0, gz=True),
           dict(name="chrA_pct01_minqual0", vcf="main", ctg_name="chrA", var_pct_full=0.1, min_qual=0, gz=False),
           dict(name="dup_pct0", vcf="dup", ctg_name="chrA", var_pct_full=0.0, min_qual=5, gz=False),
           dict(name="dup_pct05", vcf="dup", ctg_name="chrA", var_pct_full=0.5, min_qual=5, gz=False),
           dict(name="dup_pct03_gz", vcf="dup", ctg_name="chrA", var_pct_full=0.3, min_qual=5, gz=True),
           dict(name="absent_contig", vcf="main", ctg_name="chrC", var_pct_full=0.1, min_qual=5, gz=False)]


def main():
    assert os.path.isdir(REF)
    tmp = tempfile.mkdtemp(prefix="gen_select_hetero_")
    texts = {k: f() for k, f in INPUTS.items()}
    for k, t in texts.items():
        open(os.path.join(tmp, k + ".vcf"), "w").write(t)
        with gzip.open(os.path.join(tmp, k + ".vcf.gz"), "wt") as f:
            f.write(t)
    out = []
    for cf in CONFIGS:
        ns = dict(tumor_vcf_fn=cf["vcf"] + (".vcf.gz" if cf["gz"] else ".vcf"), var_pct_full=cf["var_pct_full"], ctg_name=cf["ctg_name"],
                  output_folder="out_" + cf["name"], min_qual=cf["min_qual"])
        p = subprocess.run([sys.executable, "-W", "ignore", "-c", CHILD, REF, json.dumps(ns)], cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True)
        assert p.returncode == 0, (ns, p.stderr[-3000:])
        text = open(os.path.join(tmp, ns["output_folder"], cf["ctg_name"] + ".vcf")).read()
        n = sum(1 for ln in text.split("\n") if ln and ln[0] != "#")
        print(cf["name"], n, "rows", repr(p.stdout), flush=True)
        out.append(dict(name=cf["name"], vcf=cf["vcf"], gz=cf["gz"], namespace=ns, output=text, printed=p.stdout))
    by = {o["name"]: o for o in out}
    assert by["chrA_pct0"]["output"] != by["chrA_pct05"]["output"] and by["chrA_minqual0"]["output"] != by["chrA_pct01_minqual0"]["output"]
    assert "\t1/0:" in by["chrA_pct0"]["output"] and "\t0|1:" in by["chrA_pct0"]["output"] and "\t1|0:" in by["chrA_pct0"]["output"]
    assert "\t1/1:" not in by["chrA_pct0"]["output"] and "AT\tA" not in by["chrA_pct0"]["output"] and "A,T" not in by["chrA_pct0"]["output"]
    assert "chrA\t100\t.\tA\tG" in by["dup_pct0"]["output"] and "chrA\t300\t.\tG\tT\t7" in by["dup_pct0"]["output"]
    assert "not found:0" not in by["chrA_pct0"]["printed"] and "selected: chrC: 0," in by["absent_contig"]["printed"]
    parser = json.loads(subprocess.run([sys.executable, "-c", gen_cli.PARSER_PROBE % REF, "src.select_hetero_snp_for_phasing"], stdout=subprocess.PIPE,
                                       check=True, cwd=tmp).stdout.decode().strip().split("\n")[-1])
    assert len(parser) == 5, parser
    gen_cli.dump_json_gz("select_hetero.json.gz", dict(inputs=texts, configs=out, parser=parser))
    shutil.rmtree(tmp, ignore_errors=True)
    print("wrote select_hetero.json.gz", os.path.getsize(os.path.join(HERE, "select_hetero.json.gz")), "bytes")


if __name__ == "__main__":
    main()
