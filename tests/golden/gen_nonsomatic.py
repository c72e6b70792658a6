#!/usr/bin/env python3
"""The reference's nonsomatic_tagging (STEP 3 / STEP 7 of run_clairs_to) executed on small panels of normals (build container only:
/root/reference must exist) -> nonsomatic.json.gz.

Stored, data only:
  * `parser`: the option table of the reference's parser (as gen_cli.py records the others);
  * `scenarios`: per scenario the input files (base64: the md5 of every PoN is in the output header), the argv lists in the order they ran
    (relative paths, run from the scenario's directory), and what the reference left: every output file, stdout, the exit status.
The reference runs here under CPython with the system gzip and no tabix, i.e. its full-stream path (same tags as its tabix path).
Usage: python tests/golden/gen_nonsomatic.py"""
import base64
import gzip
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gen_cli  # noqa: E402
import ponutil  # noqa: E402

HEADER = ("##fileformat=VCFv4.2\n##source=ClairS-TO\n##FILTER=<ID=PASS,Description=\"All filters passed\">\n"
          "##FILTER=<ID=NonSomatic,Description=\"Non-somatic variant tagged by panel of normals\">\n"
          "##FILTER=<ID=LowQual,Description=\"Low-quality variant\">\n##FILTER=<ID=RefCall,Description=\"Reference call\">\n"
          "##INFO=<ID=H,Number=0,Type=Flag,Description=\"Variant found only in one haplotype in the phased reads\">\n"
          "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n##contig=<ID=chr1,length=248956422>\n"
          "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n")
PON_HEADER = "##fileformat=VCFv4.2\n##source=pon\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
BASES = "ACGT"


def call_row(ctg, pos, ref, alt, flt="PASS", gt="0/1"):
    return "%s\t%d\t.\t%s\t%s\t%.4f\t%s\tFAU=3;FCU=0;FGU=0;FTU=1\tGT:GQ:DP:AF\t%s:20:30:0.2500\n" % (ctg, pos, ref, alt, 17.5, flt, gt)


def synth_calls(rng, contigs, n_per, show_ref_rows=True):
    rows, calls = [], []
    for ctg in contigs:
        pos = 100
        for _ in range(n_per):
            pos += rng.randint(3, 60)
            ref = rng.choice(BASES) if rng.random() < 0.8 else rng.choice(BASES) + rng.choice(BASES) * rng.randint(1, 3)
            alt = rng.choice([b for b in BASES if b != ref[0]]) if len(ref) == 1 or rng.random() < 0.5 else ref[0]
            r = rng.random()
            flt, gt = ("PASS", "0/1") if r < 0.6 else (("LowQual", "0/1") if r < 0.8 else (("RefCall", "0/0") if show_ref_rows else ("PASS", "1/1")))
            rows.append(call_row(ctg, pos, ref, alt, flt, gt))
            calls.append((ctg, pos, ref, alt))
    return rows, calls


def pon_lines(rng, calls, extra_contigs=(), frac=0.5):
    """PoN records: some calls exactly, some by position only (another allele), multi-ALT records, records elsewhere"""
    recs = []
    for ctg, pos, ref, alt in calls:
        r = rng.random()
        if r < frac * 0.4:
            recs.append((ctg, pos, ref, alt))
        elif r < frac * 0.7:
            recs.append((ctg, pos, ref, ",".join(rng.sample([alt, "T", "G", "AC"], 3))))
        elif r < frac:
            recs.append((ctg, pos, ref + "A", alt))
        if rng.random() < 0.5:
            recs.append((ctg, pos + rng.randint(1, 2), "A", "G"))
    for ctg in extra_contigs:
        for i in range(20):
            recs.append((ctg, 100 + 37 * i, "C", "T"))
    order = {c: i for i, c in enumerate(dict.fromkeys([c for c, _, _, _ in recs]))}
    recs.sort(key=lambda x: (order[x[0]], x[1]))
    return ["%s\t%d\trs%d\t%s\t%s\t50\tPASS\tAF=0.01\n" % (c, p, i, r, a) for i, (c, p, r, a) in enumerate(recs)]


def write_pon(d, name, text, kind, block=65280):
    """kind: vcf (plain), bgzf_tbi, bgzf, gzip (one plain gzip member), raw (bytes as given)"""
    p = os.path.join(d, name)
    if kind in ("vcf", "raw"):
        open(p, "wb").write(text)
    elif kind in ("bgzf_tbi", "bgzf"):
        ponutil.write_bgzf_vcf(p, text, with_tbi=kind == "bgzf_tbi", block=block)
    elif kind == "gzip":
        with open(p, "wb") as f:
            with gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as g:
                g.write(text)
    return name


def run_ref(argv, cwd):
    env = dict(os.environ, PYTHONPATH=REF)
    p = subprocess.run([sys.executable, os.path.join(REF, "clairs_to.py"), "nonsomatic_tagging"] + argv, cwd=cwd, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return dict(argv=argv, stdout=p.stdout.decode(), returncode=p.returncode)


def snapshot(d):
    return {os.path.relpath(os.path.join(b, f), d): base64.b64encode(open(os.path.join(b, f), "rb").read()).decode()
            for b, _, fs in os.walk(d) for f in sorted(fs)}


def scenario(tmp, name, build):
    d = os.path.join(tmp, name)
    os.makedirs(d)
    invocations = build(d)
    inputs = snapshot(d)
    runs = [run_ref(a, d) for a in invocations]
    after = snapshot(d)
    outputs = {k: v for k, v in after.items() if k not in inputs}
    print("scenario", name, len(runs), "runs,", sorted(outputs), [r["returncode"] for r in runs])
    return dict(name=name, inputs=inputs, runs=runs, outputs=outputs)


def odd_pon_text(calls):
    """the line forms of the issue: CRLF, leading whitespace, trailing tab, < 5 fields, empty lines, mid-file '#', POS 000123 / +123 / 1_23,
    non-ASCII bytes inside REF/ALT and after field 5, a record longer than 64 KiB"""
    (c0, p0, r0, a0), (c1, p1, r1, a1), (c2, p2, r2, a2), (c3, p3, r3, a3), (c4, p4, r4, a4), (c5, p5, r5, a5), (c6, p6, r6, a6), \
        (c7, p7, r7, a7), (c8, p8, r8, a8) = calls[:9]
    lines = [PON_HEADER.encode(),
             ("%s\t%d\t.\t%s\t%s\t50\tPASS\tX\r\n" % (c0, p0, r0, a0)).encode(),
             ("  \t%s\t%d\t.\t%s\t%s\t50\n" % (c1, p1, r1, a1)).encode(),
             ("%s\t%d\t.\t%s\t%s\t\n" % (c2, p2, r2, a2)).encode(),
             ("%s\t%d\t.\t%s\n" % (c3, p3, r3)).encode(),
             b"\n", b"   \n",
             ("#%s\t%d\t.\t%s\t%s\n" % (c3, p3, r3, a3)).encode(),
             ("%s\t%09d\t.\t%s\t%s\t50\n" % (c4, p4, r4, a4)).encode(),
             ("%s\t+%d\t.\t%s\t%s\t50\n" % (c5, p5, r5, a5)).encode(),
             ("%s\t%s_%s\t.\t%s\t%s\t50\n" % (c6, str(p6)[:1], str(p6)[1:], r6, a6)).encode() if len(str(p6)) > 1 else b"\n",
             ("%s\t%d\t.\t%s\t%s\xe9,%s\t50\n" % (c7, p7, r7, a7, a7)).encode("latin-1"),
             ("%s\t%d\t.\t%s\t%s\t50\tPASS\tNOTE=caf\xc3\xa9\xff\n" % (c8, p8, r8, a8)).encode("latin-1"),
             ("%s\t%d\t.\tA\tG\t50\tPASS\tAF=%s\n" % (calls[9][0], calls[9][1], "1" * 70000)).encode()]
    c, p, r, a = calls[10]
    lines.append(("%s\t%d\t.\t%s\t%s\t50\tPASS\tLONG=%s\n" % (c, p, r, a, "ACGT" * 17000)).encode())
    c, p, r, a = calls[11]
    lines.append(("%s\t%d\t.\t%s\t%s" % (c, p, r, a)).encode())              # no final newline
    return b"".join(lines)


def main():
    assert os.path.isdir(REF)
    rng = random.Random(20261016)
    tmp = tempfile.mkdtemp(prefix="gen_nonsomatic_")
    scenarios = []

    def s1(d):        # --ctg_name, four PoNs of the four kinds, matching True,True,False,False
        rows, calls = synth_calls(rng, ["chr1"], 120)
        rows2, _ = synth_calls(rng, ["chr2"], 20)
        open(os.path.join(d, "snv_pileup.vcf"), "w").write(HEADER + "".join(rows + rows2))
        pons = []
        os.makedirs(os.path.join(d, "pon"))
        for i, kind in enumerate(("vcf", "bgzf_tbi", "bgzf", "gzip")):
            text = (PON_HEADER + "".join(pon_lines(rng, calls, extra_contigs=("chr2", "chr7")))).encode()
            pons.append(write_pon(d, "pon/p%d.vcf%s" % (i + 1, "" if kind == "vcf" else ".gz"), text, kind, block=4096))
        return [["--pileup_vcf_fn", "snv_pileup.vcf", "--output_vcf_fn", "out_chr1.vcf", "--ctg_name", "chr1", "--panel_of_normals", ",".join(pons),
                 "--panel_of_normals_require_allele_matching", "True,True,False,False", "--pypy3", "pypy3", "--parallel", "parallel"]]
    scenarios.append(scenario(tmp, "ctg_four_kinds", s1))

    def s2(d):        # no --ctg_name: contig order, PoN contigs outside the input
        rows, calls = [], []
        for ctg in ("chrUn_x", "10", "chrX", "chr2", "chr1"):
            r, c = synth_calls(rng, [ctg], 25)
            rows += r
            calls += c
        open(os.path.join(d, "in.vcf"), "w").write(HEADER + "".join(rows))
        text = (PON_HEADER + "".join(pon_lines(rng, calls, extra_contigs=("chr5", "chrM")))).encode()
        write_pon(d, "a.vcf.gz", text, "bgzf_tbi", block=2048)
        write_pon(d, "b.vcf", text, "vcf")
        return [["--pileup_vcf_fn", "in.vcf", "--output_vcf_fn", "out.vcf", "--panel_of_normals", "a.vcf.gz,b.vcf",
                 "--panel_of_normals_require_allele_matching", "True,False"]]
    scenarios.append(scenario(tmp, "all_contigs", s2))

    def s3(d):        # --show_ref: RefCall rows take part; --input_filter_tag; --disable_print_nonsomatic_calls; --skip_pon_md5
        rows, calls = synth_calls(rng, ["chr3"], 80)
        open(os.path.join(d, "in.vcf"), "w").write(HEADER + "".join(rows))
        text = (PON_HEADER + "".join(pon_lines(rng, calls, frac=0.7))).encode()
        write_pon(d, "p.vcf.gz", text, "bgzf")
        base = ["--pileup_vcf_fn", "in.vcf", "--ctg_name", "chr3", "--panel_of_normals", "p.vcf.gz", "--panel_of_normals_require_allele_matching", "False"]
        return [base + ["--output_vcf_fn", "show_ref.vcf", "--show_ref"],
                base + ["--output_vcf_fn", "filter_tag.vcf", "--input_filter_tag", "PASS,RefCall", "--show_ref"],
                base + ["--output_vcf_fn", "disable_print.vcf", "--disable_print_nonsomatic_calls"],
                base + ["--output_vcf_fn", "skip_md5.vcf", "--skip_pon_md5"],
                ["--pileup_vcf_fn", "in.vcf", "--ctg_name", "chr3", "--output_vcf_fn", "no_pon.vcf"]]
    scenarios.append(scenario(tmp, "options", s3))

    def s6(d):        # odd lines, through every file kind
        _, calls = synth_calls(rng, ["chr1"], 40)
        rows = [call_row(c, p, r, a) for c, p, r, a in calls]
        open(os.path.join(d, "in.vcf"), "w").write(HEADER + "".join(rows))
        text = odd_pon_text(calls)
        write_pon(d, "odd.vcf", text, "vcf")
        write_pon(d, "odd_bgzf.vcf.gz", text, "bgzf", block=1000)
        write_pon(d, "odd_gzip.gz", text.replace(b"\r\n", b"\r"), "gzip")         # lone '\r' ends a line on the gzip path
        write_pon(d, "empty.vcf", b"", "raw")
        open(os.path.join(d, "eof_only.vcf.gz"), "wb").write(ponutil.BGZF_EOF)
        write_pon(d, "not_gzip.txt", text, "raw")
        write_pon(d, "bad_pos.vcf", (PON_HEADER + "chr9\t12a\t.\tA\tG\n").encode(), "vcf")
        all_pons = "odd.vcf,odd_bgzf.vcf.gz,odd_gzip.gz,empty.vcf,eof_only.vcf.gz,not_gzip.txt"
        return [["--pileup_vcf_fn", "in.vcf", "--ctg_name", "chr1", "--output_vcf_fn", "allele.vcf", "--panel_of_normals", all_pons,
                 "--panel_of_normals_require_allele_matching", "True,True,True,True,True,True"],
                ["--pileup_vcf_fn", "in.vcf", "--output_vcf_fn", "pos.vcf", "--panel_of_normals", all_pons,
                 "--panel_of_normals_require_allele_matching", "False,False,False,False,False,False"],
                ["--pileup_vcf_fn", "in.vcf", "--ctg_name", "chr1", "--output_vcf_fn", "bad.vcf", "--panel_of_normals", "bad_pos.vcf",
                 "--panel_of_normals_require_allele_matching", "True"],
                ["--pileup_vcf_fn", "in.vcf", "--output_vcf_fn", "bad_elsewhere.vcf", "--panel_of_normals", "bad_pos.vcf",
                 "--panel_of_normals_require_allele_matching", "True"]]
    scenarios.append(scenario(tmp, "odd_lines", s6))

    def s7(d):        # two contig invocations sharing one aggregate TSV, then the sample summary
        rows, calls = [], []
        for ctg in ("chr1", "chr2"):
            r, c = synth_calls(rng, [ctg], 40)
            rows += r
            calls += c
        open(os.path.join(d, "in.vcf"), "w").write(HEADER + "".join(rows))
        text = (PON_HEADER + "".join(pon_lines(rng, calls))).encode()
        write_pon(d, "g.vcf.gz", text, "bgzf_tbi")
        write_pon(d, "k.vcf", text, "vcf")
        out = []
        for ctg in ("chr1", "chr2"):
            out.append(["--pileup_vcf_fn", "in.vcf", "--output_vcf_fn", "nt_%s.vcf" % ctg, "--ctg_name", ctg, "--nonsomatic_summary_aggregate_tsv",
                        "vcf_output/summary.tsv", "--panel_of_normals", "g.vcf.gz,k.vcf", "--panel_of_normals_require_allele_matching", "True,False"])
        out.append(["--print_sample_nonsomatic_summary_from_tsv", "vcf_output/summary.tsv"])
        return out
    scenarios.append(scenario(tmp, "aggregate", s7))

    whole = whole_run(tmp, rng)
    import json
    import shutil
    raw = json.dumps(dict(parser=gen_cli_parser(tmp), scenarios=scenarios, whole_run=whole), separators=(",", ":"), sort_keys=True).encode()
    shutil.rmtree(tmp, ignore_errors=True)
    with open(os.path.join(HERE, "nonsomatic.json.gz"), "wb") as f:
        with gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as g:
            g.write(raw)
    print("wrote nonsomatic.json.gz", len(raw), "bytes raw")


WHOLE_PONS = ("pon/p1.vcf", "pon/p2.vcf.gz", "pon/p3.vcf.gz", "pon/p4.vcf.gz")


def whole_run(tmp, rng):
    """STEP 3 and STEP 7 as run_clairs_to builds them: `--dry_run --panel_of_normals A,B,C,D --panel_of_normals_require_allele_matching ...` on
    the ont_whole set-up of gen_cli.py, then its nonsomatic_tagging commands (GNU parallel emulated: one invocation per row of CONTIGS), the
    sort_vcf merges and the summary prints, executed by the reference on the snv_pileup.vcf / indel_pileup.vcf it wrote for that run
    (cli_run.json.gz).  Paths: @W@ = the run's directory (the commands run there), @T@ = the scratch root; the PoNs are given relative."""
    import shutil
    import clisim
    from conftest import load_json_gz
    vo = load_json_gz("cli_run.json.gz")["executed"]["ont_whole"]["vcf_output"]
    calls = []
    for name in ("snv_pileup.vcf", "indel_pileup.vcf"):
        for row in vo[name].split("\n"):
            c = row.split("\t")
            if len(c) > 7 and not row.startswith("#"):
                calls.append((c[0], int(c[1]), c[3], c[4].split(",")[0]))
    conda = gen_cli.fake_conda(tmp)
    inputs = clisim.write_inputs(os.path.join(tmp, "in"))
    models = {}
    os.makedirs(os.path.join(tmp, "models"), exist_ok=True)
    for k in ("snv_aff", "snv_neg", "indel_aff", "indel_neg", "snv_lik", "indel_lik"):   # a dry run only checks that they exist
        models[k] = os.path.join(tmp, "models", k)
        open(models[k], "w").close()
    os.makedirs(os.path.join(tmp, "pon"))
    for p, kind in zip(WHOLE_PONS, ("vcf", "bgzf_tbi", "bgzf", "gzip")):
        write_pon(tmp, p, (PON_HEADER + "".join(pon_lines(rng, calls, extra_contigs=("chr21",)))).encode(), kind, block=2048)
    flags = ["--disable_intermediate_phasing", "--panel_of_normals", ",".join(WHOLE_PONS), "--panel_of_normals_require_allele_matching",
             "True,True,False,False"]
    w, commands = gen_cli.dry_run(tmp, "ont_whole_pon", "ont_r10_dorado_sup_5khz", flags, conda, inputs, models)
    wt = os.path.join(w, "tmp")
    os.makedirs(os.path.join(wt, "vcf_output"), exist_ok=True)
    for name in ("snv_pileup.vcf", "indel_pileup.vcf"):
        open(os.path.join(wt, "vcf_output", name), "w").write(vo[name])
    shutil.copytree(os.path.join(tmp, "pon"), os.path.join(w, "pon"))
    before = set(os.listdir(os.path.join(wt, "vcf_output")))
    env = dict(os.environ, PATH=os.path.join(conda, "bin") + ":" + os.environ["PATH"], PYTHONPATH=REF)
    runs = []
    for command in commands:
        if "nonsomatic_tagging" not in command:
            continue
        for sub, argv, source in gen_cli.invocations(command):
            if sub not in ("nonsomatic_tagging", "sort_vcf"):
                continue
            rows = [None] if source is None else sorted(r for r in open(source).read().split("\n") if r.strip())
            for r in rows:
                a = argv if r is None else gen_cli.substitute(argv, [r])
                p = subprocess.run([sys.executable, os.path.join(REF, "clairs_to.py"), sub] + a, cwd=w, env=env, stdout=subprocess.PIPE,
                                   stderr=subprocess.PIPE)
                assert p.returncode == 0, (sub, a, p.stderr.decode()[-2000:])
                runs.append(dict(submodule=sub, argv=[gen_cli.norm(t, tmp, w) for t in a], stdout=gen_cli.norm(p.stdout.decode(), tmp, w)))
    assert sum(r["submodule"] == "nonsomatic_tagging" for r in runs) >= 4, runs
    outputs = {f: gen_cli.norm(open(os.path.join(wt, "vcf_output", f)).read(), tmp, w)
               for f in sorted(os.listdir(os.path.join(wt, "vcf_output"))) if f not in before}
    assert "snv_pileup_nonsomatic_tagging.vcf" in outputs and "indel_pileup_nonsomatic_tagging.vcf" in outputs, sorted(outputs)
    scratch = {os.path.relpath(os.path.join(b, f), tmp): base64.b64encode(open(os.path.join(b, f), "rb").read()).decode()
               for d in ("in", "pon") for b, _, fs in os.walk(os.path.join(tmp, d)) for f in fs if not f.startswith("t.bam")}
    print("whole run:", len(runs), "invocations,", sorted(outputs))
    return dict(commands=[gen_cli.norm(c, tmp, w) for c in commands if "nonsomatic_tagging" in c], runs=runs, scratch_files=scratch,
                contigs=gen_cli.norm(open(os.path.join(wt, "CONTIGS")).read(), tmp, w),
                pileup={k: vo[k] for k in ("snv_pileup.vcf", "indel_pileup.vcf")}, outputs=outputs)


def gen_cli_parser(tmp):
    p = subprocess.run([sys.executable, "-c", gen_cli.PARSER_PROBE % REF, "src.nonsomatic_tagging"], stdout=subprocess.PIPE, check=True, cwd=tmp)
    import json
    return json.loads(p.stdout.decode().strip().split("\n")[-1])


if __name__ == "__main__":
    main()
