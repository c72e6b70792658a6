#!/usr/bin/env python3
"""The reference's aspcf (step 5 of its Verdict chain, src/cna_germline_tagging.py:130-140), run unmodified from /root/reference on the
tables of aspcfsim.py (needs the reference checkout and scipy, which its module imports) -> aspcf.json.gz.  Stored, data only: the specs
and seeds of the inputs, a SHA-256 of each input set, the argv lists (relative paths, run from the scenario's directory), every output
file's text - or, for the large scenario, its SHA-256 - and what the child process observed.

  * `default`: the default penalty on one table whose runs hold 0, 1, 5, 6, 11, 12, 13, 899, 900, 901, 1100 and 2600 heterozygous probes
    (the `< 6` rule, the 2 * kmin gate, the first window's 900, a tail window, four windows) and 40 more under a chromosome name that comes
    back; one run carries 150 homozygous probes in a row whose logR is shifted by 0.9, and the child must see their replacement.
  * `penalty50`: --penalty 50 on a table whose level changes every ~10 heterozygous probes: the first pass must leave at least 800 distinct
    levels, so that the loop goes on to 70.
  * `no_het`: a table without a heterozygous probe: no output file.

The child process imports the module from the checkout as it is and wraps three names around it: aspcfpart (which penalties and window
lengths it saw), np.where (the three-argument call of the stretch replacement, told by its source line) and np.argmin.  Over every
np.argmin call the smallest relative gap between the minimum and the next distinct value is recorded; a minimum that occurs at two
places, or a gap under 1e-12, fails the generator: change the seed, not the condition.
Usage: python tests/golden/gen_aspcf.py"""
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, HERE)

import aspcfsim  # noqa: E402
import gen_cli  # noqa: E402

BASE = ["--tumor_logr_file", "logr.txt", "--tumor_baf_file", "baf.txt", "--germline_genotypes_file", "gg.txt",
        "--tumor_logr_pcfed_output_file", "out_LogR.txt", "--tumor_baf_pcfed_output_file", "out_BAF.txt", "--sample_name", "TUM"]
SCENARIOS = [
    dict(name="default", argv=BASE, store="text",
         spec=dict(seed=31, hom_per_het=1.5, stretch=(9, 150, 0.9),
                   chroms=[("chr1", 0, 300), ("chr2", 1, 300), ("chr3", 5, 300), ("chr4", 6, 300), ("chr5", 11, 300), ("chr6", 12, 300),
                           ("chr7", 13, 300), ("chr8", 899, 300), ("chr9", 900, 250), ("chr10", 901, 300), ("chr8", 40, 300), ("chr11", 1100, 350),
                           ("chr12", 2600, 400)])),
    dict(name="penalty50", argv=BASE + ["--penalty", "50"], store="sha256",
         spec=dict(seed=77, hom_per_het=1.5, stretch=None, chroms=[("chr1", 10200, 14), ("chr2", 8100, 14), ("chr3", 6300, 14)])),
    dict(name="no_het", argv=BASE, store="text", spec=dict(seed=5, hom_per_het=1.5, stretch=None, chroms=[("chr1", 0, 300), ("chr2", 0, 300)])),
]

CHILD = r"""
import json, linecache, sys
sys.path.insert(0, sys.argv[1])
sys.argv = ["aspcf"] + sys.argv[2:]
import numpy as np
seen = dict(gammas=[], window_lengths=[], replaced=0, argmin_calls=0, argmin_ties=0, argmin_gap=None)
argmin, where = np.argmin, np.where
def spy_argmin(a, *args, **kw):
    a = np.asarray(a)
    seen["argmin_calls"] += 1
    if a.size > 1:
        mn = a.min()
        if int((a == mn).sum()) > 1:
            seen["argmin_ties"] += 1
        else:
            nxt = a[a > mn].min()
            gap = float((nxt - mn) / max(abs(mn), abs(nxt)))
            if seen["argmin_gap"] is None or gap < seen["argmin_gap"]:
                seen["argmin_gap"] = gap
    return argmin(a, *args, **kw)
def spy_where(c, *args, **kw):
    if len(args) == 2:
        f = sys._getframe(1)
        if "pcfed2" in linecache.getline(f.f_code.co_filename, f.f_lineno):
            seen["replaced"] += int(np.sum(c))
    return where(c, *args, **kw)
np.argmin, np.where = spy_argmin, spy_where
import aspcf as m
part = m.aspcfpart
def spy_part(**kw):
    if kw["gamma"] not in seen["gammas"]:
        seen["gammas"].append(kw["gamma"])
    if kw["gamma"] == seen["gammas"][0]:
        seen["window_lengths"].append(len(kw["logRpart"]))
    return part(**kw)
m.aspcfpart = spy_part
m.main()
print("SEEN " + json.dumps(seen))
"""


def run_ref(d, argv):
    p = subprocess.run([sys.executable, "-c", CHILD, os.path.join(REF, "src", "verdict")] + argv, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True)
    assert p.returncode == 0, (argv, p.stderr[-3000:])
    return json.loads([ln for ln in p.stdout.split("\n") if ln.startswith("SEEN ")][-1][5:])


def main():
    assert os.path.isdir(REF)
    tmp = tempfile.mkdtemp(prefix="gen_aspcf_")
    out = []
    for sc in SCENARIOS:
        d = os.path.join(tmp, sc["name"])
        os.makedirs(d)
        files = aspcfsim.tables(sc["spec"])
        for k, v in files.items():
            open(os.path.join(d, k), "w").write(v)
        seen = run_ref(d, sc["argv"])
        outputs = {}
        for fn in ("out_LogR.txt", "out_BAF.txt"):
            if os.path.exists(os.path.join(d, fn)):
                text = open(os.path.join(d, fn)).read()
                outputs[fn] = text if sc["store"] == "text" else hashlib.sha256(text.encode()).hexdigest()
                if fn == "out_LogR.txt":
                    seen["levels"] = len({r.split("\t")[2] for r in text.split("\n")[1:] if r})
        print(sc["name"], {k: len(v) for k, v in outputs.items()}, seen if len(seen["window_lengths"]) < 40 else dict(seen, window_lengths="..."), flush=True)
        assert seen["argmin_ties"] == 0, seen
        assert seen["argmin_gap"] is None or seen["argmin_gap"] >= 1e-12, seen
        if sc["name"] == "default":
            assert seen["gammas"] == [1000] and seen["replaced"] > 5, seen
            assert {6, 11, 12, 13, 40, 899, 900, 1000} <= set(seen["window_lengths"]), sorted(set(seen["window_lengths"]))
            assert seen["window_lengths"].count(1000) >= 2 and len(outputs) == 2
        elif sc["name"] == "penalty50":
            assert seen["gammas"][:2] == [50, 70] and len(outputs) == 2, seen
        else:
            assert not outputs and seen["gammas"] == [] and seen["argmin_calls"] == 0
        out.append(dict(name=sc["name"], argv=sc["argv"], store=sc["store"], spec=sc["spec"], inputs_sha256=aspcfsim.digest(files), outputs=outputs,
                        seen=seen))
    gen_cli.dump_json_gz("aspcf.json.gz", dict(scenarios=out))
    shutil.rmtree(tmp, ignore_errors=True)
    print("wrote aspcf.json.gz", os.path.getsize(os.path.join(HERE, "aspcf.json.gz")), "bytes")


if __name__ == "__main__":
    main()
