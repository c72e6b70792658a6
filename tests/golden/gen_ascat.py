#!/usr/bin/env python3
"""The reference's run_ascat (step 6 of its Verdict chain, src/cna_germline_tagging.py:143-164), run unmodified from /root/reference on the
tables of ascatsim.py (needs the reference checkout) -> ascat.json.gz.  Stored, data only: the specs and seeds of the inputs, a SHA-256 of
each input set, the argv lists (relative paths, run from the scenario's directory), every output file's text, what the child printed and
what it observed.

  * `default`: an aberrant genome at purity 0.4 whose optimum comes from the first scan; between 150 and 400 segments; a chromosome name
    that comes back; runs of equal logR without a heterozygous probe inside (the lookup 10000 rows around); neighbouring runs that merge.
  * `fallback`: a genome without a lost allele, so that the first scan accepts nothing.  That scan has by then overwritten every cell it
    visited with the largest value of the cell's window, so the three later scans, which run on what is left, find no local minimum
    either: the "Could not find" branch, its message on stdout and no output file.
  * `bounds`: --min_ploidy 1.6 --max_ploidy 4.8 --gamma 0.55: a matrix of 84 ploidies.
  * `no_het`: a table without a heterozygous probe: no output file.

The child process imports the module from the checkout as it is.  It wraps create_distance_matrix (the matrix's shape, the number of
segments) and follows run_ascat's own frame line by line: which of the four `optima.append` lines ran (the scan that filled the list), how
many optima there were and the relative gap between the two smallest when the choice is made, how often the far lookup ran, how many
merges the first round made.  A gap under 1e-12 fails the generator: change the seed, not the condition.
Usage: python tests/golden/gen_ascat.py"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, HERE)

import ascatsim  # noqa: E402
import gen_cli  # noqa: E402

BASE = ["--tumor_logr_file", "logr.txt", "--tumor_baf_file", "baf.txt", "--germline_genotypes_file", "gg.txt", "--tumor_logr_segmented_file", "seg_logr.txt",
        "--tumor_baf_segmented_file", "seg_baf.txt", "--tumor_purity_ploidy_output_file", "out_Purity_Ploidy.txt", "--tumor_cna_output_file", "out_CNA.txt",
        "--sample_name", "TUM"]
OUTPUTS = ("out_Purity_Ploidy.txt", "out_CNA.txt")
ABERRANT = [(1, 1, 25), (2, 1, 25), (2, 0, 15), (1, 0, 10), (2, 2, 10), (3, 1, 10), (3, 2, 5)]
COMMON = dict(het=(3, 30), hom_per_het=1.2, noise=(0.01, 0.004), hom_run=(25, 0.35))
SCENARIOS = [
    dict(name="default", argv=BASE,
         spec=dict(COMMON, seed=11, purity=0.4, ploidy=2.8, gamma=1.0, states=ABERRANT, hom_runs=[17, 140],
                   chroms=[("chr1", 40), ("chr2", 35), ("chr3", 30), ("chr1", 12), ("chr4", 45), ("chr5", 38), ("chrX", 30)])),
    dict(name="fallback", argv=BASE,
         spec=dict(COMMON, seed=23, purity=0.6, ploidy=2.2, gamma=1.0, states=[(1, 1, 75), (2, 1, 25)], hom_runs=[],
                   chroms=[("chr1", 30), ("chr2", 30), ("chr3", 20)])),
    dict(name="bounds", argv=BASE + ["--min_ploidy", "1.6", "--max_ploidy", "4.8", "--gamma", "0.55"],
         spec=dict(COMMON, seed=37, purity=0.55, ploidy=3.1, gamma=0.55, states=ABERRANT, hom_runs=[5],
                   chroms=[("chr1", 40), ("chr2", 40), ("chr3", 40)])),
    dict(name="no_het", argv=BASE,
         spec=dict(COMMON, seed=5, purity=0.4, ploidy=2.0, gamma=1.0, states=[(1, 1, 1)], hom_runs=[], het=(0, 0), chroms=[("chr1", 20), ("chr2", 20)])),
]

CHILD = r"""
import json, linecache, sys
sys.path.insert(0, sys.argv[1])
sys.argv = ["run_ascat"] + sys.argv[2:]
import numpy as np
import run_ascat as m
seen = dict(matrix_shape=None, S=None, scan=0, optima=0, gap=None, far_lookups=0, merges_first_round=0)
cdm = m.create_distance_matrix
def spy(segments, gamma, **kw):
    d = cdm(segments, gamma, **kw)
    seen["matrix_shape"], seen["S"] = list(d.shape), int(segments.shape[0])
    return d
m.create_distance_matrix = spy
code = m.run_ascat.__code__
src = linecache.getlines(code.co_filename)
def lines_with(text):
    return [i + 1 for i, ln in enumerate(src) if text in ln]
appends, choice, far, merge = lines_with("optima.append("), lines_with("optlim = np.min(localmin)"), lines_with("start - 10000"), lines_with("skipnext = True")
assert len(appends) == 4 and len(choice) == 1 and len(far) == 1 and len(merge) == 1, (appends, choice, far, merge)
rounds = [0]
def local(frame, event, arg):
    if event == "line":
        ln = frame.f_lineno
        if ln in appends:
            seen["scan"] = appends.index(ln) + 1
        elif ln == choice[0]:
            ms = sorted(float(o[0]) for o in frame.f_locals["optima"])
            seen["optima"] = len(ms)
            if len(ms) > 1:
                seen["gap"] = (ms[1] - ms[0]) / max(abs(ms[0]), abs(ms[1])) if ms[1] != ms[0] else 0.0
        elif ln == far[0]:
            seen["far_lookups"] += 1
        elif ln == merge[0] and frame.f_locals["_"] == 0:
            seen["merges_first_round"] += 1
    return local
def tracer(frame, event, arg):
    return local if frame.f_code is code else None
sys.settrace(tracer)
m.main()
sys.settrace(None)
print("SEEN " + json.dumps(seen))
"""


def run_ref(d, argv):
    p = subprocess.run([sys.executable, "-W", "ignore", "-c", CHILD, os.path.join(REF, "src", "verdict")] + argv, cwd=d, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, (argv, p.stderr[-3000:])
    lines = p.stdout.split("\n")
    seen = [ln for ln in lines if ln.startswith("SEEN ")][-1]
    return json.loads(seen[5:]), "".join(ln + "\n" for ln in lines if ln and not ln.startswith("SEEN "))


def main():
    assert os.path.isdir(REF)
    tmp = tempfile.mkdtemp(prefix="gen_ascat_")
    out = []
    for sc in SCENARIOS:
        d = os.path.join(tmp, sc["name"])
        os.makedirs(d)
        files = ascatsim.tables(sc["spec"])
        for k, v in files.items():
            open(os.path.join(d, k), "w").write(v)
        seen, printed = run_ref(d, sc["argv"])
        outputs = {fn: open(os.path.join(d, fn)).read() for fn in OUTPUTS if os.path.exists(os.path.join(d, fn))}
        print(sc["name"], {k: len(v) for k, v in outputs.items()}, seen, repr(printed), outputs.get(OUTPUTS[0], "").split("\n")[1:2], flush=True)
        assert seen["gap"] is None or seen["gap"] >= 1e-12, seen
        names = [c[0] for c in sc["spec"]["chroms"]]
        if sc["name"] == "default":
            assert seen["scan"] == 1 and 150 <= seen["S"] <= 400 and seen["matrix_shape"] == [100, 95] and len(outputs) == 2, seen
            assert seen["far_lookups"] >= 1 and seen["merges_first_round"] >= 1 and len(set(names)) < len(names), seen
            assert sc["spec"]["purity"] == 0.4
        elif sc["name"] == "fallback":
            assert seen["scan"] == 0 and not outputs and printed == "Could not find an optimal purity and ploidy value for TUM!\n", (seen, printed)
        elif sc["name"] == "bounds":
            assert seen["matrix_shape"][0] == 84 and seen["scan"] >= 1 and len(outputs) == 2, seen
        else:
            assert not outputs and seen["matrix_shape"] is None and printed == "", seen
        out.append(dict(name=sc["name"], argv=sc["argv"], spec=sc["spec"], inputs_sha256=ascatsim.digest(files), outputs=outputs, printed=printed, seen=seen))
    gen_cli.dump_json_gz("ascat.json.gz", dict(scenarios=out))
    shutil.rmtree(tmp, ignore_errors=True)
    print("wrote ascat.json.gz", os.path.getsize(os.path.join(HERE, "ascat.json.gz")), "bytes")


if __name__ == "__main__":
    main()
