#!/usr/bin/env python3
"""The reference's compare_vcf (src/compare_vcf.py), run from the reference checkout in a child process on one generated case
-> compare_vcf.json.gz.  Each configuration is an argv handed to the reference's own main(); the Namespace its parser makes of it, what it
printed, its --output_fn, --roc_fn and the four VCFs of --output_dir are stored, with the input texts and the reference's option table.
Only data is stored.

The case: a few hundred truth records and calls over chr1, chr2 and chr3 - matches, allele and genotype mismatches, insertions,
deletions, multi-allelic rows, MNPs, an unsorted stretch and a repeated key in each file, `PASS;HighConf` and other truth rows, H in INFO,
QUALs that repeat and straddle integers; a BED (chr1, chr2; chr3 is not named) with a zero-length row, two overlapping rows and keys on,
one before and one after the two ends of an interval; two stratification BEDs, and one that names no contig of the run; a phase file and
a low-AF file.  `minaf_bam` runs --min_af with --tumor_bam_fn on the case of tests/calafutil.py with the samtools stand-in of
gen_cal_af.py, so that cal_af is the reference's own.
Usage: python tests/golden/gen_compare_vcf.py"""
import gzip
import json
import os
import random
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import calafutil  # noqa: E402
import gen_cal_af  # noqa: E402
import gen_cli  # noqa: E402

SEED = 20261020
CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import src.compare_vcf as m
ref = m.compare_vcf
def seen(args):
    sys.stderr.write("NAMESPACE " + json.dumps(vars(args)) + "\n")
    return ref(args)
m.compare_vcf = seen
sys.argv = ["compare_vcf"] + json.loads(sys.argv[2])
m.main()
"""
HEAD = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n"
QUALS = ["3", "3.5", "7.99", "8", "8.01", "8", "12.25", "12.25", "20", "0.5", "31.9", "32"]
ALLELES = [("A", "C")] * 6 + [("A", "G"), ("A", "ACG"), ("A", "AT"), ("ATG", "A"), ("AC", "A"), ("AT", "GC"), ("A", "C,T"), ("A", "AT,C")]
BED = [("chr1", 200, 400), ("chr1", 380, 500), ("chr1", 600, 600), ("chr1", 800, 1500), ("chr2", 100, 900), ("chr2", 1200, 1201)]
EDGE = [200, 201, 400, 500, 501, 600, 601, 602, 800, 801, 1500, 1501]       # chr1 keys around the interval ends


def make_texts():
    rng = random.Random(SEED)
    truth, calls, phase, lowaf = [], [], [], []
    trow = lambda c, p, r, a, flt, gt: "%s\t%d\t.\t%s\t%s\t.\t%s\t.\tGT\t%s\n" % (c, p, r, a, flt, gt)
    crow = lambda c, p, r, a, q, flt, info, gt, af: "%s\t%d\t.\t%s\t%s\t%s\t%s\t%s\tGT:GQ:DP:AF\t%s:%d:%d:%.4f\n" % (c, p, r, a, q, flt, info, gt, 10, 30, af)
    for ctg in ("chr1", "chr2", "chr3"):
        pos = sorted(set(list(range(110, 1700, 13)) + (EDGE if ctg == "chr1" else [])))
        for p in pos:
            ref, alt = ("A", "C") if p in EDGE else rng.choice(ALLELES)
            flt = rng.choice(("PASS;HighConf", "PASS;HighConf", "PASS;HighConf", "PASS;MedConf", "PASS"))
            gt = rng.choice(("0/1", "0/1", "1/1", "1|0", "0/0"))
            truth.append(trow(ctg, p, ref, alt, flt, gt))
            u = rng.random()
            if u < 0.65 or p in EDGE:
                a2, g2 = alt, gt
                v = rng.random()
                if v < 0.15:
                    a2 = {"C": "T", "G": "T"}.get(alt, alt + "A" if len(alt) > 1 and "," not in alt else "G")
                elif v < 0.3:
                    g2 = "1/1" if gt != "1/1" else "0/1"
                calls.append(crow(ctg, p, ref, a2, rng.choice(QUALS), rng.choice(("PASS", "PASS", "PASS", "PASS", "LowQual")), rng.choice((".", "H", "H;X", "X")),
                                  g2, rng.choice((0.02, 0.08, 0.2, 0.45, 0.9))))
            if rng.random() < 0.3:                                 # a call of its own between two truth positions
                r2, a2 = rng.choice(ALLELES)
                calls.append(crow(ctg, p + 5, r2, a2, rng.choice(QUALS), "PASS", rng.choice((".", "H")), "0/1", rng.choice((0.02, 0.3))))
            # rows of the phase / low-AF files: ctg pos depth alt h0 h1 h2 a0 a1 a2
            hp = rng.choice(("0 3 0 1 9 8", "0 0 4 2 7 9", "0 2 2 0 5 5", "0 0 0 3 0 6", "1 1 0 0 4 4"))
            phase.append("%s %d %d %d %s\n" % (ctg, p, 30, rng.choice((0, 1, 2, 3, 9)), hp))
            lowaf.append("%s %d %d %d %s\n" % (ctg, p, rng.choice((0, 20, 30)), rng.choice((0, 1, 2, 3, 9)), hp))
    for rows in (truth, calls):
        a = len(rows) // 3
        rows[a:a + 12] = rows[a:a + 12][::-1]                      # an unsorted stretch
    # a repeated key in each file: the first place, the last row
    truth.append(trow("chr1", 149, "A", "T", "PASS;HighConf", "0/1"))
    truth.append(trow("chr1", 162, "A", "T", "PASS", "1/1"))
    first = calls[0].split("\t")
    calls.append(crow(first[0], int(first[1]), "A", "G", "8", "PASS", "H", "0/1", 0.5))
    calls.append(crow("chr2", 400, "A", "C", ".", "LowQual", ".", "0/1", 0.5))        # a QUAL that is no number: in `nobed` only, which has no sweep
    return HEAD + "".join(truth), HEAD + "".join(calls), "".join(phase), "".join(lowaf)


def bed_text(rows, comment=True):
    return ("#chrom\tstart\tend\n" if comment else "") + "".join("%s\t%d\t%d\n" % r for r in rows)


IN, OUT = "@IN@", "@OUT@"
BASE = ["--truth_vcf_fn", IN + "/truth.vcf", "--input_vcf_fn", IN + "/input.vcf"]
DEMO = BASE + ["--bed_fn", IN + "/fp.bed", "--output_dir", OUT + "/benchmark", "--input_filter_tag", "PASS", "--ctg_name", "chr1", "--ctg_start", "150",
               "--ctg_end", "1600"]
ALL = ["--truth_vcf_fn", IN + "/truth.vcf.gz", "--input_vcf_fn", IN + "/input.vcf", "--bed_fn", IN + "/fp.bed", "--output_dir", OUT + "/benchmark",
       "--input_filter_tag", "PASS"]
FILES = ["--output_fn", OUT + "/table.txt"]
CONFIGS = [
    ("demo", DEMO),
    ("all_ctg", ALL),
    ("nobed", BASE + ["--output_dir", OUT + "/benchmark"] + FILES),
    ("strat2", ALL + ["--strat_bed_fn", IN + "/strat_a.bed," + IN + "/strat_b.bed.gz"]),
    ("strat_empty", ALL + ["--strat_bed_fn", IN + "/strat_none.bed"]),
    ("gt", ALL + ["--skip_genotyping", "False"] + FILES),
    ("bi", ALL + ["--benchmark_indel"] + FILES),
    ("bi_hc", ALL + ["--benchmark_indel", "--high_confident_only", "True"]),
    ("bi_gt_strat", ALL + ["--benchmark_indel", "--skip_genotyping", "False", "--strat_bed_fn", IN + "/strat_a.bed", "--truth_filter_tag", "PASS;HighConf,PASS"]),
    ("best_int", ALL + ["--output_best_f1_score"]),
    ("best_frac", ALL + ["--output_best_f1_score", "--use_int_cut_off", "False"] + FILES),
    ("best_debug", DEMO + ["--output_best_f1_score", "--debug"]),
    ("bi_best_debug", ALL + ["--benchmark_indel", "--output_best_f1_score", "--debug"]),
    ("roc", ALL + ["--roc_fn", OUT + "/roc.txt"]),
    ("minqual", ALL + ["--min_qual", "3.5", "--max_qual", "20", "--roc_fn", OUT + "/roc.txt"]),
    ("lowaf_file", ALL + ["--min_af", "0.05", "--low_af_path", IN + "/lowaf.txt"]),
    ("lowaf_file_ctg", DEMO + ["--min_af", "0.1", "--low_af_path", IN + "/lowaf.txt", "--min_alt_coverage", "1"]),
    ("phase1", ALL + ["--validate_phase_only", "1", "--phase_output", IN + "/phase.txt"]),
    ("phase2", DEMO + ["--validate_phase_only", "2", "--phase_output", IN + "/phase.txt", "--benchmark_indel"]),
    ("minaf_bam", ["--truth_vcf_fn", IN + "/cal_truth.vcf", "--input_vcf_fn", IN + "/cal_input.vcf", "--tumor_bam_fn", "@BAM@", "--samtools", "@SAMTOOLS@",
                   "--min_af", "0.3", "--ctg_name", "chrB", "--truth_filter_tag", "PASS", "--threads", "4", "--output_dir", OUT + "/benchmark"]),
]


def run_ref(tmp, argv):
    p = subprocess.run([sys.executable, "-W", "ignore", "-c", CHILD, REF, json.dumps(argv)], cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, (argv, p.stderr[-3000:])
    ns = [ln for ln in p.stderr.split("\n") if ln.startswith("NAMESPACE ")][-1]
    return json.loads(ns[10:]), p.stdout


def main():
    assert os.path.isdir(REF)
    tmp = tempfile.mkdtemp(prefix="gen_compare_vcf_")
    truth, calls, phase, lowaf = make_texts()
    cal_truth, cal_input = calafutil.vcf_texts()
    inputs = {"truth.vcf": truth, "truth.vcf.gz": truth, "input.vcf": calls, "phase.txt": phase, "lowaf.txt": lowaf, "fp.bed": bed_text(BED),
              "strat_a.bed": bed_text([("chr1", 100, 1000), ("chr2", 0, 700), ("chr3", 300, 1300)], comment=False),
              "strat_b.bed.gz": bed_text([("chr1", 300, 1600), ("chr2", 500, 1700)]),
              "strat_none.bed": bed_text([("chrUn", 0, 100000)]), "cal_truth.vcf": cal_truth, "cal_input.vcf": cal_input}
    os.makedirs(os.path.join(tmp, "in"))
    for name, text in inputs.items():
        with (gzip.open(os.path.join(tmp, "in", name), "wt") if name.endswith(".gz") else open(os.path.join(tmp, "in", name), "w")) as f:
            f.write(text)
    # the samtools stand-in of gen_cal_af.py, and a file under the BAM's name (the reference only asks whether it exists)
    c = calafutil.case()
    rows = {}
    for text in (cal_truth, cal_input):
        for ln in text.split("\n"):
            if ln and ln[0] != "#":
                ctg, pos = ln.split("\t")[:2]
                for hp in (0, 1):
                    rows["%s:%s:%d" % (ctg, pos, hp)] = calafutil.mpileup_row(c["entered"][ctg], ctg, int(pos), bool(hp))
    json.dump(rows, open(os.path.join(tmp, "rows.json"), "w"))
    tool = os.path.join(tmp, "samtools")
    open(tool, "w").write(gen_cal_af.STAND_IN % sys.executable)
    os.chmod(tool, 0o755)
    open(os.path.join(tmp, "t.bam"), "w").close()
    out = []
    for name, argv in CONFIGS:
        o = os.path.join(tmp, "out_" + name)
        os.makedirs(o)
        real = [a.replace(IN, os.path.join(tmp, "in")).replace(OUT, o).replace("@BAM@", "t.bam").replace("@SAMTOOLS@", tool) for a in argv]
        ns, stdout = run_ref(tmp, real)
        files = {}
        for base, _, fs in os.walk(o):
            for f in fs:
                files[os.path.relpath(os.path.join(base, f), o)] = open(os.path.join(base, f)).read()
        ns = {k: (v.replace(os.path.join(tmp, "in"), IN).replace(o, OUT).replace(tool, "samtools") if isinstance(v, str) else v) for k, v in ns.items()}
        out.append(dict(name=name, argv=argv, namespace=ns, stdout=stdout, files=files))
        print(name, repr(stdout[-260:]), {k: v.count("\n") for k, v in files.items()}, flush=True)
    by = {o["name"]: o for o in out}
    rows_of = lambda name, f: [ln.split("\t") for ln in by[name]["files"]["benchmark/" + f].split("\n") if ln]
    table = lambda name: {ln.split()[0]: ln.split()[1:] for ln in (by[name]["files"].get("table.txt") or by[name]["stdout"]).split("\n") if ln[:3] in ("SNV", "IND", "INS", "DEL")}
    # every branch is reached
    for name in ("demo", "all_ctg", "bi", "bi_hc"):
        assert all(rows_of(name, f) for f in ("fp.vcf", "fn.vcf", "fp_fn.vcf", "tp.vcf")), name
    assert all(int(x) > 0 for k in ("SNV",) for x in table("demo")[k][3:6])
    assert all(int(x) > 0 for k in ("INS", "DEL") for x in table("bi")[k][3:6]), table("bi")
    assert table("bi")["SNV"][3:5] == ["0", "0"] and int(table("bi")["SNV"][5]) > 0      # the SNV calls are deleted from the input dict
    assert any(len(r[3]) != len(r[4]) for r in rows_of("bi_hc", "tp.vcf")) and table("bi_hc") != table("bi")
    demo_pos = {int(r[1]) for f in ("fp.vcf", "fn.vcf", "fp_fn.vcf", "tp.vcf") for r in rows_of("demo", f)}
    assert {201, 500, 601} & demo_pos and not {200, 501, 600, 602} & demo_pos      # on, before and after an interval's ends; the widened row
    assert 400 in demo_pos                                         # inside the second of two overlapping rows only
    assert not any(r[0] == "chr3" for f in ("fp.vcf", "fn.vcf", "tp.vcf") for r in rows_of("all_ctg", f))      # a contig the BED does not name
    assert any(r[0] == "chr3" for r in rows_of("nobed", "fn.vcf")) and any(r[0] == "chr2" for r in rows_of("all_ctg", "tp.vcf"))
    assert "Genotype mismatch count/Total fp_fn count: 0/" not in by["gt"]["stdout"] and "Genotype mismatch" in by["gt"]["stdout"]
    assert table("gt") != table("all_ctg") and table("strat2") != table("all_ctg") and table("minqual") != table("all_ctg")
    assert table("strat_empty")["SNV"][3:6] == ["0", "0", "0"] and "truth records: 0" in by["strat_empty"]["stdout"]
    assert table("lowaf_file") != table("all_ctg") and table("phase1") != table("all_ctg") and table("phase1") != table("phase2")
    assert by["best_int"]["stdout"].count("SNV(Best F1)") == 1 and by["best_frac"]["files"]["table.txt"].count("SNV(Best F1)") == 1
    dbg = [ln.split() for ln in by["best_debug"]["stdout"].split("SNV(Best F1)")[1].split("\n")[2:] if ln]
    assert len(dbg) >= 5 and len({r[4] for r in dbg}) > 2, dbg      # several cut-offs with different TP counts: `>=` against `>` shows
    roc = [ln.split("\t") for ln in by["roc"]["files"]["roc.txt"].split("\n") if ln]
    assert len(roc) >= 8 and any("." in r[0] and not r[0].endswith(".0") for r in roc)
    assert "[INFO] Total truth need to calculate AF:" in by["minaf_bam"]["stdout"] and table("minaf_bam")["SNV"][3] != "0"
    assert any(ln.split("\t")[1] == "149" and ln.split("\t")[4] == "T" for ln in truth.split("\n")[2:] if ln)
    parser = json.loads(subprocess.run([sys.executable, "-c", gen_cli.PARSER_PROBE % REF, "src.compare_vcf"], stdout=subprocess.PIPE, check=True,
                                       cwd=tmp).stdout.decode().strip().split("\n")[-1])
    assert len(parser) == 34, len(parser)
    gen_cli.dump_json_gz("compare_vcf.json.gz", dict(seed=SEED, inputs=inputs, configs=out, parser=parser))
    shutil.rmtree(tmp, ignore_errors=True)
    size = os.path.getsize(os.path.join(HERE, "compare_vcf.json.gz"))
    print("wrote compare_vcf.json.gz", size, "bytes")
    assert size < os.path.getsize(os.path.join(HERE, "region2k.json.gz"))


if __name__ == "__main__":
    main()
