#!/usr/bin/env python3
"""The reference's add_back_missing_variants_in_genotyping (src/add_back_missing_variants_in_genotyping.py), run from the reference checkout
in a child process on generated texts -> add_back.json.gz.  Each configuration is an argv handed to the reference's own main(); the Namespace
its parser makes of it, what it printed, the bytes of --output_fn and whether `<call_fn>.bak` exists are stored, with the input texts and
the reference's option table.  Only data is stored.  bgzip and tabix are absent where this runs, so --output_fn stays plain.

The texts (a few hundred rows in all): calls and a list over chr1, 1, chrX and one contig outside the major list, each with a repeated key,
an unsorted stretch and a `#` line in mid-file; list rows of 5, 8, 10 and 12 columns, a multi-base and an empty REF, a space-separated row;
hybrid_info rows whose ref_base overrides, equals or is empty, the depth-seqs fields `30-A 3 C 5`, `30-`, `30-A 3 -AC 2`, `x-A 1`, `30-A x`,
a repeated base key and an empty field, a row of three columns and a key no list row has; variants of the calls and the list whose last
line has no newline; a list in which every row is called, and one that is a header only.

Every configuration runs under two PYTHONHASHSEED values and the stored bytes must agree: no case rests on the reference's set order.
Usage: python tests/golden/gen_add_back.py"""
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

import gen_cli  # noqa: E402

SEED = 20261021
CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import src.add_back_missing_variants_in_genotyping as m
ref = m.genotype_vcf
def seen(args):
    sys.stderr.write("NAMESPACE " + json.dumps(vars(args)) + "\n")
    return ref(args)
m.genotype_vcf = seen
sys.argv = ["add_back_missing_variants_in_genotyping"] + json.loads(sys.argv[2])
m.main()
"""
HEAD = "##fileformat=VCFv4.2\n##source=test\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n"
CONTIGS = ("chr1", "1", "chrX", "chrUn_KI270742v1")
BASES = "ACGT"


def call_row(c, p, ref, alt, q="12.5", flt="PASS"):
    return "%s\t%d\t.\t%s\t%s\t%s\t%s\tH\tGT:GQ:DP:AF\t0/1:%d:%d:%.4f\n" % (c, p, ref, alt, q, flt, 12, 30, 0.25)


def list_row(c, p, ref, alt, cols=8):
    full = [c, str(p), "rs%d" % p, ref, alt, "50", "PASS", "AC=1", "GT", "0/1", "extra1", "extra2"]
    return "\t".join(full[:cols]) + "\n"


def make_texts():
    rng = random.Random(SEED)
    calls, listed, info = [], [], {"chr1.1_hybrid_info": [], "chrX.2_hybrid_info": []}
    info_file = lambda c: "chr1.1_hybrid_info" if c in ("chr1", "1") else "chrX.2_hybrid_info"
    for c in CONTIGS:
        for p in range(100, 100 + 17 * 24, 17):
            ref, alt = rng.choice(BASES), rng.choice(BASES)
            listed.append(list_row(c, p, ref, alt, rng.choice((5, 8, 10, 12))))
            if rng.random() < 0.35:
                calls.append(call_row(c, p, ref, alt))
            if rng.random() < 0.2:
                calls.append(call_row(c, p + 3, ref, alt, flt="LowQual"))          # a call the list does not name
            if rng.random() < 0.85:
                cnt = " ".join("%s %d" % (b, rng.randrange(0, 40)) for b in rng.sample(BASES, rng.randrange(1, 5)))
                info[info_file(c)].append("%s\t%d\t%s\t%d-%s\n" % (c, p, rng.choice((ref, ref, "N", "")), rng.randrange(0, 90), cnt))
    # hand-made list rows at positions no call has, one per shape
    special = [
        ("chr1", 21, list_row("chr1", 21, "ATG", "A", 10), "A", "30-A 3 C 5"),                  # multi-base REF, ref_base equals its first base
        ("chr1", 22, "chr1\t22\t.\t\tC\t.\t.\t.\n", "G", "30-"),                                 # empty REF, ref_base overrides
        ("chr1", 23, list_row("chr1", 23, "C", "T", 12), "", "30-A 3 -AC 2"),                    # empty ref_base; three '-' parts
        ("chr1", 24, list_row("chr1", 24, "C", "T", 5), "T", "x-A 1"),
        ("chr1", 25, list_row("chr1", 25, "C", "T", 8), "C", "30-A x"),
        ("chr1", 26, list_row("chr1", 26, "C", "T", 8), "CA", "41-A 1 C 2 A 7 G 0 T 123456789"),  # a repeated base key; a long ref_base
        ("chr1", 27, list_row("chr1", 27, "G", "T", 12), "G", ""),                                # an empty field
        ("chr1", 28, "chr1 28 . G T\n", "G", "9-G 9"),                                            # space-separated: key by whitespace, columns by tab
        ("chr1", 29, list_row("chr1", 29, "G", "T", 10), None, None),                             # an info row of three columns
        ("chr1", 30, list_row("chr1", 30, "G", "T", 10), "A", "007-A 05 N 3 T"),                  # leading zeros, an unpaired key
        ("1", 31, "1\t31\n", "A", "12-AC 4 C 1"),
    ]
    for c, p, row, ref_base, field in special:
        listed.append(row)
        info[info_file(c)].append("%s\t%d\tG\n" % (c, p) if field is None else "%s\t%d\t%s\t%s\textra\n" % (c, p, ref_base, field))
    info["chrX.2_hybrid_info"].append("chrX\t99999\tA\t5-A 5\n")                                   # a key no list row has
    info["chr1.1_hybrid_info"].append("chr1\t21\tA\t30-A 3 C 5\n")                                 # a repeated info key, the same values
    for rows in (calls, listed):
        a = len(rows) // 3
        rows[a:a + 9] = rows[a:a + 9][::-1]                                                        # an unsorted stretch
        rows.insert(2 * len(rows) // 3, "#a comment in mid-file\n")
    # a repeated key in each file: the first place, the last row
    calls.append(call_row(calls[0].split("\t")[0], int(calls[0].split("\t")[1]), "A", "G", q="99"))
    listed.append(list_row("chr1", 22, "TT", "C", 8))
    listed.append(list_row("chrX", 98, "A", "C", 10))                                          # the last row: no call has it
    calls_text, list_text = HEAD + "".join(calls), HEAD + "".join(listed)
    called_keys = sorted({tuple(r.split("\t")[:2]) for r in calls if r[0] != "#"})
    all_called = HEAD + "".join(list_row(c, int(p), "A", "C", 8) for c, p in called_keys[::2])
    return dict(calls=calls_text, calls_nonl=calls_text[:-1], list=list_text, list_nonl=list_text[:-1], list_called=all_called, list_header=HEAD,
                info={k: "".join(v) for k, v in info.items()})


D = "@D@"
G, HY = "--genotyping_mode_vcf_fn", "--hybrid_mode_vcf_fn"
IO = ["--call_fn", D + "/calls.vcf", "--output_fn", D + "/out.vcf"]
CAND = ["--candidates_folder", D + "/cand"]
CONFIGS = [
    ("geno_sw", [G, D + "/list.vcf"] + IO + CAND + ["--switch_genotype", "True"]),
    ("geno_nosw", [G, D + "/list.vcf"] + IO + CAND + ["--switch_genotype", "False"]),
    ("hyb_sw", [HY, D + "/list.vcf"] + IO + CAND + ["--switch_genotype", "True"]),
    ("hyb_nosw", [HY, D + "/list.vcf"] + IO + CAND + ["--switch_genotype", "no"]),
    ("both", [G, D + "/list.vcf", HY, D + "/list_called.vcf"] + IO + CAND),
    ("geno_none_str", [G, "None", HY, D + "/list.vcf"] + IO + CAND),
    ("both_none", [G, "None"] + IO + CAND),
    ("default_switch", [G, D + "/list.vcf"] + IO + CAND),
    ("no_folder", [G, D + "/list.vcf"] + IO),
    ("bad_folder", [HY, D + "/list.vcf"] + IO + ["--candidates_folder", D + "/nowhere"]),
    ("calls_gz", [G, D + "/list.vcf", "--call_fn", D + "/calls.vcf.gz", "--output_fn", D + "/out.vcf"] + CAND),
    ("calls_gz_hyb", [HY, D + "/list.vcf", "--call_fn", D + "/calls.vcf.gz", "--output_fn", D + "/out.vcf"]),
    ("calls_missing", [G, D + "/list.vcf", "--call_fn", D + "/absent.vcf", "--output_fn", D + "/out.vcf"] + CAND),
    ("calls_missing_hyb", [HY, D + "/list.vcf", "--call_fn", D + "/absent.vcf", "--output_fn", D + "/out.vcf", "--switch_genotype", "f"]),
    ("list_gz", [G, D + "/list.vcf.gz"] + IO + CAND),
    ("nonl_geno", [G, D + "/list_nonl.vcf", "--call_fn", D + "/calls_nonl.vcf", "--output_fn", D + "/out.vcf"] + CAND),
    ("nonl_hyb", [HY, D + "/list_nonl.vcf", "--call_fn", D + "/calls_nonl.vcf", "--output_fn", D + "/out.vcf", "--switch_genotype", "False"]),
    ("all_called_geno", [G, D + "/list_called.vcf"] + IO + CAND),
    ("all_called_hyb", [HY, D + "/list_called.vcf"] + IO + CAND),
    ("header_only_geno", [G, D + "/list_header.vcf"] + IO + CAND),
    ("header_only_hyb", [HY, D + "/list_header.vcf"] + IO + CAND),
    ("list_missing", [G, D + "/absent_list.vcf"] + IO + CAND),
]


def write_inputs(d, texts):
    """the files a configuration's argv names, fresh in directory d"""
    os.makedirs(os.path.join(d, "cand"))
    plain = {"calls.vcf": "calls", "calls_nonl.vcf": "calls_nonl", "list.vcf": "list", "list_nonl.vcf": "list_nonl", "list_called.vcf": "list_called",
             "list_header.vcf": "list_header"}
    for name, key in plain.items():
        with open(os.path.join(d, name), "w") as f:
            f.write(texts[key])
    for name, key in (("calls.vcf.gz", "calls"), ("list.vcf.gz", "list")):
        with gzip.open(os.path.join(d, name), "wt") as f:
            f.write(texts[key])
    for name, text in texts["info"].items():
        with open(os.path.join(d, "cand", name), "w") as f:
            f.write(text)
    with open(os.path.join(d, "cand", "chr1.1_snv"), "w") as f:          # not a hybrid_info file: never read
        f.write("chr1\t21\tA\t1-A 1\n")


def run_ref(tmp, name, argv, texts, seed):
    d = os.path.join(tmp, "%s_%s" % (name, seed))
    write_inputs(d, texts)
    real = [a.replace(D, d) for a in argv]
    env = dict(os.environ, PYTHONHASHSEED=str(seed))
    p = subprocess.run([sys.executable, "-W", "ignore", "-c", CHILD, REF, json.dumps(real)], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       env=env)
    ns = [ln for ln in p.stderr.split("\n") if ln.startswith("NAMESPACE ")]
    ns = {k: (v.replace(d, D) if isinstance(v, str) else v) for k, v in json.loads(ns[-1][10:]).items()} if ns else None
    out_fn = os.path.join(d, "out.vcf")
    call_fn = real[real.index("--call_fn") + 1]
    exit_msg = None
    if p.returncode != 0:
        exit_msg = [ln for ln in p.stderr.split("\n") if ln.startswith("[ERROR]")]
        assert exit_msg, (name, p.stderr[-3000:])
        exit_msg = exit_msg[-1]
    return dict(name=name, argv=argv, namespace=ns, stdout=p.stdout, exit=exit_msg, output=open(out_fn).read() if os.path.exists(out_fn) else None,
                bak=os.path.exists(call_fn + ".bak"), compressed=os.path.exists(out_fn + ".gz"))


def main():
    assert os.path.isdir(REF)
    tmp = tempfile.mkdtemp(prefix="gen_add_back_")
    texts = make_texts()
    out = []
    for name, argv in CONFIGS:
        a, b = run_ref(tmp, name, argv, texts, 1), run_ref(tmp, name, argv, texts, 4242)
        assert a == b, "%s rests on the reference's set order" % name
        assert not a["compressed"]
        out.append(a)
        print(name, repr(a["stdout"] or a["exit"]), None if a["output"] is None else a["output"].count("\n"), a["bak"], flush=True)
    by = {o["name"]: o for o in out}
    # every branch is reached
    sw = by["geno_sw"]["output"]
    for want in ("chr1\t21\trs21\tA\t.\t.\t.\t.\tGT:DP:AU:CU:GU:TU\t./.:30:3:5:0:0\n", "chr1\t22\trs22\tG\t.", "./.:30:0:0:0:0\n",
                 "chr1\t26\trs26\tCA\t.\t.\t.\t.\tGT:DP:AU:CU:GU:TU\t./.:41:7:2:0:123456789\n", "chr1 28 . G T\t.\t.\tG\t.", "./.:9:0:0:9:0\n",
                 "./.:7:5:0:0:0\n", "1\t31\t.\tA\t.", "\textra1\textra2\n"):
        assert want in sw, want
    assert sw.count("./.:0:0:0:0:0") >= 5 and sw.startswith(HEAD + "#a comment in mid-file\n")
    assert by["both"]["output"] == sw and by["default_switch"]["output"] == sw and by["calls_gz"]["output"] == sw and by["list_gz"]["output"] == sw
    assert by["geno_none_str"]["output"] == by["hyb_sw"]["output"] != sw
    assert by["both_none"]["exit"].startswith("[ERROR] Both VCF") and by["both_none"]["output"] is None
    assert "./." not in by["geno_nosw"]["output"].replace(HEAD, "") and by["no_folder"]["output"] != sw
    assert by["calls_missing"]["bak"] is False and by["geno_sw"]["bak"] is True and by["calls_missing"]["output"][0] != "#"
    assert "calls: 0, added" in by["calls_missing"]["stdout"] and ", added 0 variants" in by["all_called_geno"]["stdout"]
    assert by["nonl_geno"]["output"].count("\n") == sw.count("\n") - 1 and "0.2500chr" in by["nonl_geno"]["output"]      # the calls' last row, mid-file
    assert "\tGT\t0/1chrX\t" in by["nonl_hyb"]["output"]                                                # the list's last row, kept, mid-file
    order = [ln.split()[0] for ln in by["hyb_sw"]["output"].split("\n") if ln and ln[0] != "#"]
    assert [c for k, c in enumerate(order) if k == 0 or order[k - 1] != c] == ["chr1", "chrX", "1", "chrUn_KI270742v1"], order
    parser = json.loads(subprocess.run([sys.executable, "-c", gen_cli.PARSER_PROBE % REF, "src.add_back_missing_variants_in_genotyping"], stdout=subprocess.PIPE,
                                       check=True, cwd=tmp).stdout.decode().strip().split("\n")[-1])
    assert len(parser) == 6, len(parser)
    gen_cli.dump_json_gz("add_back.json.gz", dict(seed=SEED, texts=texts, configs=out, parser=parser))
    shutil.rmtree(tmp, ignore_errors=True)
    size = os.path.getsize(os.path.join(HERE, "add_back.json.gz"))
    print("wrote add_back.json.gz", size, "bytes")
    assert size < 200000


if __name__ == "__main__":
    main()
