#!/usr/bin/env python3
"""The reference's postfilter_variants (STEP 4-2 / 8-2 of run_clairs_to for short reads), run unmodified from /root/reference on the simulated
contigs of pfsim.py (needs the reference checkout) -> postfilter.json.gz.

Neither samtools nor GNU parallel is needed: `samtools` is pfsim.SHIM_SAMTOOLS (mpileup serves eight-column rows, faidx the FASTA) and
`parallel` the stand-in of gen_hapfilter_wide.py.  Inputs are regenerated from the seeds by the tests and pinned by SHA-256; stored, data only:
  * `parser`: the option table of the reference's parser; `argv`: the postfilter_variants argv lists of the ilmn dry runs of argv.json.gz;
  * `scenarios`: per scenario its spec, the digest of its input files and its runs: the argv (relative paths, run from the scenario's directory),
    the output VCF (or the link target), PF_INFO_*, stdout, and whether the reference's two modes (the default: one process per call under
    `parallel`; chunk mode) wrote the same VCF; `per_pos`: a few `--pos` invocations and the line each printed;
  * `fisher` / `entropy`: values of the reference's fisher_exact and calculate_sequence_entropy.
The coverage the issue asks for is asserted on the reference's output before anything is written (and again by the tests).
  * `whole_run`: the STEP 4-2 / 8-2 command lines of an ilmn `run_clairs_to --dry_run` on clisim's set-up; their postfilter_variants and
    postprocess_vcf invocations executed by the reference, in order, on realignment VCFs of two simulated contigs (no --ctg_name, the default
    one-process-per-call mode), down to the post-processed snv.vcf / indel.vcf.
Usage: python tests/golden/gen_postfilter.py"""
import json
import os
import random
import stat
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gen_cli  # noqa: E402
import pfsim  # noqa: E402
from gen_hapfilter_wide import SHIM_PARALLEL  # noqa: E402

BASE = ["--tumor_bam_fn", "t.bam", "--ref_fn", "ref.fa", "--samtools", "./samtools", "--threads", "4"]


def run_spec(name, mode, extra, ctg=None, both_modes=False):
    argv = BASE + ["--pileup_vcf_fn", "in_%s.vcf" % mode, "--output_vcf_fn", ("out/%s.vcf" if name != "off" else "%s.vcf") % name, "--output_dir", "work_%s" % name]
    if ctg:
        argv += ["--ctg_name", ctg]
    if mode == "indel":
        argv.append("--is_indel")
    return dict(name=name, mode=mode, argv=argv + extra, both_modes=both_modes)


SCENARIOS = [
    dict(name="main", spec=dict(contigs=[("chr1", 11), ("chr2", 12), ("chr20", 13)]),
         runs=[run_spec("%s_%s" % (c, m), m, [], ctg=c, both_modes=True) for c in ("chr1", "chr2", "chr20") for m in ("snv", "indel")]),
    dict(name="options", spec=dict(contigs=[("chrA", 21), ("chrB.alt", 22)]),
         runs=[run_spec("no_ctg_snv", "snv", []), run_spec("no_ctg_indel", "indel", []),
               run_spec("show_ref", "snv", ["--show_ref"], ctg="chrA"),
               run_spec("filter_tag", "snv", ["--input_filter_tag", "PASS"], ctg="chrA"),
               run_spec("filter_tag_ref", "snv", ["--input_filter_tag", "PASS,RefCall", "--show_ref"], ctg="chrB.alt"),
               run_spec("no_rse", "snv", ["--disable_read_start_end_filtering", "True"], ctg="chrA"),
               run_spec("cov3", "snv", ["--min_alt_coverage", "3"], ctg="chrA"),
               run_spec("flank50", "snv", ["--flanking", "50"], ctg="chrA"),
               run_spec("flank50_indel", "indel", ["--flanking", "50"], ctg="chrA"),
               run_spec("off", "snv", ["--enable_postfilter", "False"], ctg="chrA"),
               run_spec("test_pos", "snv", ["--test_pos", "@POS@"], ctg="chrA")]),
    dict(name="odd", spec=dict(contigs=[("chrO", 31)], odd=True),
         runs=[run_spec("odd_snv", "snv", [], ctg="chrO", both_modes=True), run_spec("odd_indel", "indel", [], ctg="chrO")]),
]


def write_scenario(d, spec):
    files = pfsim.scenario_files(spec)
    os.makedirs(d, exist_ok=True)
    for k, v in files.items():
        open(os.path.join(d, k), "w").write(v)
    open(os.path.join(d, "t.bam"), "w").close()
    for name, text in (("samtools", pfsim.SHIM_SAMTOOLS), ("parallel", SHIM_PARALLEL)):
        fn = os.path.join(d, name)
        open(fn, "w").write(text)
        os.chmod(fn, os.stat(fn).st_mode | stat.S_IEXEC)
    return files


def fill_test_pos(argv, files):
    """@POS@ = the 5th PASS call of in_snv.vcf"""
    if "@POS@" not in argv:
        return argv
    rows = [r.split("\t") for r in files["in_snv.vcf"].split("\n") if r and r[0] != "#" and r.split("\t")[6] == "PASS" and r.startswith("chrA\t")]
    return [rows[4][1] if t == "@POS@" else t for t in argv]


def run_ref(d, argv, chunk):
    extra = ["--parallel", "./parallel", "--pypy3", sys.executable] + (["--postfilter_variants_chunk_mode", "True"] if chunk else [])
    p = subprocess.run([sys.executable, os.path.join(REF, "clairs_to.py"), "postfilter_variants"] + argv + extra, cwd=d,
                       env=dict(os.environ, PYTHONPATH=REF, PYTHONHASHSEED="0"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, (argv, p.stderr[-3000:])
    return p.stdout


def collect(d, argv):
    out_fn = os.path.join(d, argv[argv.index("--output_vcf_fn") + 1])
    work = os.path.join(d, argv[argv.index("--output_dir") + 1])
    info = [f for f in sorted(os.listdir(work)) if f.startswith("PF_INFO")] if os.path.isdir(work) else []
    rec = dict(link=os.readlink(out_fn) if os.path.islink(out_fn) else None, out_vcf=None if os.path.islink(out_fn) else open(out_fn).read(),
               pf_info={f: open(os.path.join(work, f)).read() for f in info})
    os.remove(out_fn)
    if os.path.dirname(out_fn) != d:
        os.rmdir(os.path.dirname(out_fn))                       # every run finds the output folder missing (VcfWriter says so on stdout)
    return rec


def tags_of(vcf_text):
    """[(set of the four tags, SB text)] of the evaluated rows"""
    out = []
    for r in vcf_text.split("\n"):
        c = r.split("\t")
        if len(c) > 7 and r[0] != "#" and ";SB=" in c[7]:
            out.append((set(c[6].split(";")) & {"ReadStartEnd", "VariantCluster", "StrandBias", "LowSeqEntropy"}, c[7].rsplit(";SB=", 1)[1]))
    return out


def check_coverage(scenarios):
    ev = [t for s in scenarios for r in s["runs"] if r["out_vcf"] for t in tags_of(r["out_vcf"])]
    n = len(ev)
    stats = dict(evaluated=n, two_or_more=sum(len(t) >= 2 for t, _ in ev), sb_exponent=sum("e" in sb for _, sb in ev),
                 sb_plain=sum("e" not in sb for _, sb in ev))
    for tag in ("ReadStartEnd", "VariantCluster", "StrandBias", "LowSeqEntropy"):
        stats[tag] = sum(tag in t for t, _ in ev)
    print("coverage:", stats)
    assert n >= 300, stats
    for tag in ("ReadStartEnd", "VariantCluster", "StrandBias", "LowSeqEntropy"):
        assert stats[tag] >= 10 and n - stats[tag] >= 10, (tag, stats)
    assert stats["two_or_more"] >= 5 and stats["sb_exponent"] >= 1 and stats["sb_plain"] >= 1, stats
    return stats


def scalars():
    """the reference's Fisher test and sequence entropy on seeded inputs"""
    sys.path.insert(0, REF)
    from src.postfilter_variants import calculate_sequence_entropy, fisher_exact
    rng = random.Random(7)
    tables = [(0, 0, 0, 0), (3, 3, 3, 3), (0, 5, 0, 7), (12, 0, 0, 9), (1, 0, 0, 0)]
    tables += [tuple(rng.randint(0, m) for _ in range(4)) for m in (4, 12, 40, 120, 400) for _ in range(12)]
    fisher = [dict(table=t, p=repr(fisher_exact([[t[0], t[1]], [t[2], t[3]]])), rounded=str(round(fisher_exact([[t[0], t[1]], [t[2], t[3]]]), 5)))
              for t in tables]
    seqs = ["A" * 33, "AC" * 16 + "A", "ACGT" * 8 + "A", "A" * 20, "ACGTN" * 6 + "RYK"]
    seqs += ["".join(rng.choice("ACGT" if k % 3 else "AC") for _ in range(33)) for k in range(20)]
    entropy = [dict(seq=s, value=repr(calculate_sequence_entropy(sequence=s, entropy_window=33))) for s in seqs]
    return fisher, entropy


WHOLE_SPEC = dict(contigs=[("chr20", 41), ("chr21", 42)])
PYPY3 = "#!/bin/sh\nexec %s \"$@\"\n"


def whole_run(tmp):
    """@W@ = the run's directory (the commands run there), @T@ = the scratch root.  The dry run is clisim's ilmn set-up; for the execution
    in/ref.fa(.fai) become the simulated contigs' (same names), mp.txt in @W@ feeds the samtools stand-in, and the two realignment VCFs -
    what realign_variants would have left - are the simulated calls."""
    import clisim
    conda = gen_cli.fake_conda(tmp)
    inputs = clisim.write_inputs(os.path.join(tmp, "in"))
    models = {}
    os.makedirs(os.path.join(tmp, "models"), exist_ok=True)
    for k in ("snv_aff", "snv_neg", "indel_aff", "indel_neg", "snv_lik", "indel_lik"):   # a dry run only checks that they exist
        models[k] = os.path.join(tmp, "models", k)
        open(models[k], "w").close()
    w, commands = gen_cli.dry_run(tmp, "ilmn_whole_postfilter", "ilmn", [], conda, inputs, models)
    commands = [c for c in commands if " postfilter_variants " in c or " postprocess_vcf " in c]
    files = pfsim.scenario_files(WHOLE_SPEC)
    open(inputs["ref"], "w").write(files["ref.fa"])
    open(inputs["ref"] + ".fai", "w").write(files["ref.fa.fai"])
    vo = os.path.join(w, "tmp", "vcf_output")
    os.makedirs(vo, exist_ok=True)
    open(os.path.join(w, "mp.txt"), "w").write(files["mp.txt"])
    for mode in ("snv", "indel"):
        open(os.path.join(vo, "%s_pileup_realignment.vcf" % mode), "w").write(files["in_%s.vcf" % mode])
    bin_dir = os.path.join(tmp, "bin")
    os.makedirs(bin_dir)
    for name, text in (("samtools", pfsim.SHIM_SAMTOOLS), ("parallel", SHIM_PARALLEL), ("pypy3", PYPY3 % sys.executable)):
        fn = os.path.join(bin_dir, name)
        open(fn, "w").write(text)
        os.chmod(fn, os.stat(fn).st_mode | stat.S_IEXEC)
    before = {os.path.relpath(os.path.join(b, f), w) for b, _, fs in os.walk(w) for f in fs}
    env = dict(os.environ, PATH=bin_dir + ":" + os.environ["PATH"], PYTHONPATH=REF, PYTHONHASHSEED="0")
    runs = []
    for command in commands:
        for sub, argv, source in gen_cli.invocations(command):
            if sub not in ("postfilter_variants", "postprocess_vcf"):
                continue
            assert source is None, (sub, source)
            p = subprocess.run([sys.executable, os.path.join(REF, "clairs_to.py"), sub] + argv, cwd=w, env=env, stdout=subprocess.PIPE,
                               stderr=subprocess.PIPE, text=True)
            assert p.returncode == 0, (sub, argv, p.stderr[-3000:])
            runs.append(dict(submodule=sub, argv=[gen_cli.norm(t, tmp, w) for t in argv], stdout=gen_cli.norm(p.stdout, tmp, w)))
    assert sorted(r["submodule"] for r in runs) == ["postfilter_variants"] * 2 + ["postprocess_vcf"] * 2, [r["submodule"] for r in runs]
    outputs = {}
    for b, _, fs in os.walk(w):
        for f in sorted(fs):
            rel = os.path.relpath(os.path.join(b, f), w)
            if rel not in before:
                fn = os.path.join(b, f)
                outputs[rel] = dict(link=gen_cli.norm(os.readlink(fn), tmp, w)) if os.path.islink(fn) else dict(text=gen_cli.norm(open(fn).read(), tmp, w))
    assert "snv.vcf" in outputs and "indel.vcf" in outputs and "tmp/vcf_output/snv_pileup_filtering.vcf" in outputs, sorted(outputs)
    n_tagged = sum(r.count(";SB=") for r in (outputs["snv.vcf"]["text"], outputs["indel.vcf"]["text"]))
    print("whole run:", [r["submodule"] for r in runs], sorted(outputs), "rows with SB in the final VCFs:", n_tagged)
    assert n_tagged >= 100
    present = {rel: gen_cli.norm(open(os.path.join(w, rel)).read(), tmp, w) for rel in ("tmp/CMD",) if os.path.exists(os.path.join(w, rel))}
    return dict(commands=[gen_cli.norm(c, tmp, w) for c in commands], spec=WHOLE_SPEC, inputs_sha256=pfsim.digest(files), runs=runs, outputs=outputs,
                run_files=present)


def main():
    assert os.path.isdir(REF)
    tmp = tempfile.mkdtemp(prefix="gen_postfilter_")
    out_scenarios = []
    n_chunk_calls, chunk_seconds = 0, 0.0
    for sc in SCENARIOS:
        d = os.path.join(tmp, sc["name"])
        files = write_scenario(d, sc["spec"])
        rec = dict(name=sc["name"], spec=sc["spec"], inputs_sha256=pfsim.digest(files), runs=[], per_pos=[])
        for run in sc["runs"]:
            argv = fill_test_pos(run["argv"], files)
            t0 = time.time()
            stdout_chunk = run_ref(d, argv, chunk=True)
            dt = time.time() - t0
            got = collect(d, argv)
            if got["out_vcf"]:
                n_chunk_calls += len(tags_of(got["out_vcf"]))
                chunk_seconds += dt
            same = None
            if run["both_modes"]:
                stdout_default = run_ref(d, argv, chunk=False)
                got_default = collect(d, argv)
                same = got_default == got and stdout_default == stdout_chunk
                got = got_default
                stdout_chunk = stdout_default
            rec["runs"].append(dict(name=run["name"], mode=run["mode"], argv=argv, stdout=stdout_chunk, same_in_both_modes=same, **got))
            print(sc["name"], run["name"], "evaluated", len(tags_of(got["out_vcf"] or "")), "same in both modes:", same, flush=True)
        for mode in ("snv", "indel"):                           # the per-position form on a few calls of each pass
            ctg = sc["spec"]["contigs"][0][0]
            rows = [r.split("\t") for r in files["in_%s.vcf" % mode].split("\n") if r and r[0] != "#" and r.startswith(ctg + "\t")]
            for c in rows[:40:7]:
                argv = BASE + ["--ctg_name", ctg, "--pos", c[1], "--ref_base", c[3], "--alt_base", c[4], "--af", "0.25", "--qual", c[5], "--flanking", "100",
                               "--min_mq", "20", "--min_bq", "0", "--min_alt_coverage", "2", "--disable_read_start_end_filtering", "False"]
                argv += ["--is_indel"] if mode == "indel" else []
                argv += ["--enable_postfilter", "False"]
                rec["per_pos"].append(dict(argv=argv, stdout=run_ref(d, argv, chunk=False)))
        out_scenarios.append(rec)
    whole = whole_run(os.path.join(tmp, "whole"))
    stats = check_coverage(out_scenarios)
    fisher, entropy = scalars()
    p = subprocess.run([sys.executable, "-c", gen_cli.PARSER_PROBE % REF, "src.postfilter_variants"], stdout=subprocess.PIPE, check=True, cwd=tmp)
    parser = json.loads(p.stdout.decode().strip().split("\n")[-1])
    from conftest import load_json_gz
    argv = [dict(run=r["name"], argv=inv["argv"], source=inv["source"]) for r in load_json_gz("argv.json.gz")["runs"] for inv in r["invocations"]
            if inv["submodule"] == "postfilter_variants"]
    assert len(argv) >= 2, argv
    rate = dict(calls=n_chunk_calls, seconds=round(chunk_seconds, 3), calls_per_second=round(n_chunk_calls / chunk_seconds, 1),
                how="the reference under CPython, one process in chunk mode, samtools stand-in included")
    print("reference rate:", rate)
    gen_cli.dump_json_gz("postfilter.json.gz", dict(parser=parser, argv=argv, scenarios=out_scenarios, whole_run=whole, fisher=fisher, entropy=entropy, coverage=stats,
                                                    reference_rate=rate))
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)
    print("wrote postfilter.json.gz", os.path.getsize(os.path.join(HERE, "postfilter.json.gz")), "bytes")


if __name__ == "__main__":
    main()
