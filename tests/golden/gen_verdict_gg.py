#!/usr/bin/env python3
"""The reference's get_logr_and_baf and predict_germline_genotypes (steps 2 and 4 of its Verdict chain, src/cna_germline_tagging.py:92-127),
run unmodified from /root/reference on the tables of verdictsim.py (needs the reference checkout; numpy is the only third-party library
the two modules import) -> verdict_gg.json.gz.  Stored, data only: the specs and seeds of the inputs, a SHA-256 of each input set, the
argv lists (relative paths, run from the scenario's directory) and every output file's text.

  * `counts`: three contigs of the major list in --contig_fn (not in sorted order), one listed contig that is not in the major list, one
    major contig whose files exist and that --contig_fn does not list; tumour-only and with a normal.  get_logr_and_baf seeds `random`
    with int(time()) when it is imported: each run re-seeds it with the run's `seed` after the import, which is what our --seed restates.
  * `gg`: one BAF table whose runs have 0, 1, 5, 6, 7, 12, 101, 102, 300, 2 * CTO_GG_TILE + 3 = 131, 40 (a chromosome name that comes back) and
    1700 undecided probes under the default options, run with the defaults, --segmentLength 7 and 2, proportions that make extraHetero <= 0,
    a --maxHomozygous above the quantile, and the normal-BAF branch.

Every tumour-only run is checked before anything is written: the distances the reference hands to np.argsort are observed (np.argsort is
wrapped in the child process; the module itself is untouched) and sorted(dist)[e - 1] < sorted(dist)[e] must hold strictly at the cut e
(numpy's default argsort is not stable and differs by CPU: equal distances across the cut would make the expected file depend on the
machine that wrote it).  The default run must also have an infinite distance and both genotype values in every run of more than five
undecided probes.  If a seed violates a condition, change the seed, not the condition.
Usage: python tests/golden/gen_verdict_gg.py"""
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
import verdictsim  # noqa: E402

COUNTS_SPEC = dict(seed=101, rows=150, contigs=["chr1", "chr2", "chr3", "chrX", "chrUn_KI270742v1"],
                   contig_fn=["chr2", "chrUn_KI270742v1", "chr1", "chrX", "chrM"])
COUNTS_BASE = ["--tumor_allele_counts_file_prefix", "tumor_", "--alleles_file_prefix", "alleles_", "--contig_fn", "contigs.txt",
               "--tumor_logr_output_file", "out_LogR.txt", "--tumor_baf_output_file", "out_BAF.txt", "--sample_name", "TUM"]
COUNTS_RUNS = [dict(name="tumour_only", seed=12345, argv=COUNTS_BASE),
               dict(name="with_normal", seed=7, argv=COUNTS_BASE + ["--normal_allele_counts_file_prefix", "normal_", "--normal_baf_output_file", "out_NBAF.txt",
                                                                    "--normal_sample_name", "NORM"])]

GG_SPEC = dict(seed=2024, runs=[("chr1", 0), ("chr2", 1), ("chr3", 5), ("chr4", 6), ("chr5", 7), ("chr6", 12), ("chr7", 101), ("chr8", 102),
                                ("chr9", 300), ("chr10", 131), ("chr9", 40), ("chr11", 1700)])
GG_BASE = ["--tumor_logr_file", "logr.txt", "--tumor_baf_file", "baf.txt", "--germline_genotypes_output_file", "out_GG.txt", "--sample_name", "TUM"]
GG_RUNS = [dict(name="defaults", argv=GG_BASE),
           dict(name="segment7", argv=GG_BASE + ["--segmentLength", "7"]),
           dict(name="segment2", argv=GG_BASE + ["--segmentLength", "2"]),
           dict(name="no_extra_hetero", argv=GG_BASE + ["--proportionHetero", "0.1", "--proportionOpen", "0.4"]),
           dict(name="max_homozygous", argv=GG_BASE + ["--maxHomozygous", "0.46", "--proportionHetero", "0.15"]),
           dict(name="normal_baf", argv=GG_BASE + ["--normal_baf_file", "normal_baf.txt"])]

# the child process: the module is imported from the checkout as it is; np.argsort only reports what it is given
CHILD = r"""
import json, random, sys
sys.path.insert(0, sys.argv[1])
module, seed = sys.argv[2], sys.argv[3]
sys.argv = [module] + sys.argv[4:]
import numpy as np
seen = []
argsort = np.argsort
def spy(a, *args, **kw):
    seen.append([float(v) for v in a])
    return argsort(a, *args, **kw)
np.argsort = spy
m = __import__(module)
if seed != "-":
    random.seed(int(seed))
m.main()
print("SEEN " + json.dumps([[repr(v) for v in s] for s in seen]))
"""


def run_ref(d, module, argv, seed=None):
    p = subprocess.run([sys.executable, "-c", CHILD, os.path.join(REF, "src", "verdict"), module, "-" if seed is None else str(seed)] + argv, cwd=d,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, (argv, p.stderr[-3000:])
    line = [ln for ln in p.stdout.split("\n") if ln.startswith("SEEN ")][-1]
    return [[float(v) for v in s] for s in json.loads(line[5:])]


def outputs(d, argv):
    out = {}
    for flag in ("--tumor_logr_output_file", "--tumor_baf_output_file", "--normal_baf_output_file", "--germline_genotypes_output_file"):
        if flag in argv:
            fn = os.path.join(d, argv[argv.index(flag) + 1])
            out[argv[argv.index(flag) + 1]] = open(fn).read()
            os.remove(fn)
    return out


def runs_of(text):
    """[(chromosome name, [flags])] per stretch of equal names of a genotype table"""
    out = []
    for row in text.split("\n")[1:]:
        if row:
            c = row.split("\t")
            if not out or out[-1][0] != c[0]:
                out.append((c[0], []))
            out[-1][1].append(c[2])
    return out


def main():
    assert os.path.isdir(REF)
    tmp = tempfile.mkdtemp(prefix="gen_verdict_gg_")
    d = os.path.join(tmp, "counts")
    os.makedirs(d)
    files = verdictsim.count_files(COUNTS_SPEC)
    for k, v in files.items():
        open(os.path.join(d, k), "w").write(v)
    counts = dict(spec=COUNTS_SPEC, inputs_sha256=verdictsim.digest(files), runs=[])
    for run in COUNTS_RUNS:
        run_ref(d, "get_logr_and_baf", run["argv"], run["seed"])
        out = outputs(d, run["argv"])
        rows = out["out_BAF.txt"].count("\n") - 1
        chroms = [r.split("\t")[0] for r in out["out_BAF.txt"].split("\n")[1:] if r]
        assert sorted(set(chroms), key=chroms.index) == ["chr2", "chr1", "chrX"], set(chroms)
        assert 200 < rows < 3 * COUNTS_SPEC["rows"], rows
        print("counts", run["name"], "rows", rows, flush=True)
        counts["runs"].append(dict(name=run["name"], seed=run["seed"], argv=run["argv"], outputs=out))
    assert counts["runs"][0]["outputs"]["out_BAF.txt"] != counts["runs"][1]["outputs"]["out_BAF.txt"]

    d = os.path.join(tmp, "gg")
    os.makedirs(d)
    files = verdictsim.baf_files(GG_SPEC)
    for k, v in files.items():
        open(os.path.join(d, k), "w").write(v)
    gg = dict(spec=GG_SPEC, inputs_sha256=verdictsim.digest(files), runs=[])
    for run in GG_RUNS:
        seen = run_ref(d, "predict_germline_genotypes", run["argv"])
        out = outputs(d, run["argv"])
        text = out["out_GG.txt"]
        rec = dict(name=run["name"], argv=run["argv"], outputs=out, cut=None)
        if "--normal_baf_file" not in run["argv"]:
            n_false = text.count("\tFalse\n")
            assert len(seen) == (1 if n_false else 0), (run["name"], len(seen), n_false)
            if seen:
                dist = sorted(seen[0])
                assert 0 < n_false <= len(dist)
                if n_false < len(dist):
                    assert dist[n_false - 1] < dist[n_false], (run["name"], dist[n_false - 1], dist[n_false])
                    rec["cut"] = dict(extra_hetero=n_false, undecided=len(dist), below=repr(dist[n_false - 1]), above=repr(dist[n_false]),
                                      infinite=sum(v == float("inf") for v in dist))
            else:
                assert run["name"] == "no_extra_hetero"
        print("gg", run["name"], "False rows", text.count("\tFalse\n"), "of", text.count("\n") - 1, "cut", rec["cut"], flush=True)
        gg["runs"].append(rec)
    by_name = {r["name"]: r for r in gg["runs"]}
    dflt = by_name["defaults"]
    assert dflt["cut"]["undecided"] == sum(m for _, m in GG_SPEC["runs"]) and dflt["cut"]["infinite"] >= 1, dflt["cut"]
    got_runs = runs_of(dflt["outputs"]["out_GG.txt"])
    assert [c for c, _ in got_runs] == [c for c, _ in GG_SPEC["runs"]]
    for (ctg, m), (_, flags) in zip(GG_SPEC["runs"], got_runs):
        if m > 5:
            assert "True" in flags and "False" in flags, (ctg, m)
        if m == 0:
            assert set(flags) == {"True"}, ctg
    assert "False" not in by_name["no_extra_hetero"]["outputs"]["out_GG.txt"]
    assert by_name["max_homozygous"]["cut"]["undecided"] < dflt["cut"]["undecided"]       # the quantile was overridden
    assert len({r["outputs"]["out_GG.txt"] for r in gg["runs"]}) == len(gg["runs"])       # every option changes the answer

    gen_cli.dump_json_gz("verdict_gg.json.gz", dict(counts=counts, gg=gg))
    shutil.rmtree(tmp, ignore_errors=True)
    print("wrote verdict_gg.json.gz", os.path.getsize(os.path.join(HERE, "verdict_gg.json.gz")), "bytes")


if __name__ == "__main__":
    main()
