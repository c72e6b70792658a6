#!/usr/bin/env python3
"""The reference's correct_logr (step 3 of its Verdict chain, src/cna_germline_tagging.py:167-197), run unmodified from /root/reference on
the tables of correctlogrsim.py (needs the reference checkout, scipy, scikit-learn and mpmath) -> correct_logr.json.gz.  Stored, data
only: the specs and seeds of the inputs, a SHA-256 of each input set, the argv lists (relative paths, run from the scenario's directory),
the output file's text, the exit status and what the child observed.

  * `default`: about 3000 probes over several chromosome names, G = 18, T = 12, the annotation rows shuffled, rows for loci that the
    logR table lacks.
  * `repeats`: repeated keys in all three files.
  * `constant_column`: GC column 3 is constant, its correlation NaN; np.argmax takes the first NaN, so GC column 2 is chosen.
  * `narrow`: G = 8, T = 1: a second window of one entry (column 7), one replication-timing column.
  * `missing_key`: a logR key that the GC table lacks: the reference's KeyError, a non-zero exit status and no output file.

The child process imports the module from the checkout as it is.  It wraps LinearRegression.fit (the design X and y exactly as built, the
rank scikit-learn found) and np.corrcoef (row 0 of both matrices).  From them it records the three chosen columns, the relative gap
between the two largest entries of each argmax window (None where the window has one entry or a NaN decides), and `truth`: the residuals
of that X and y in 200-bit arithmetic (mpmath), as decimal strings of 25 digits - the minimum-norm least-squares solution the reference
asks LAPACK for: the centred 15 x 15 Gram matrix, its eigenvalues below 1e-12 of the largest dropped (exactly three: every block of five
sums to one), the pseudo-inverse applied to X'y.  `ref_err` = max |the reference's printed residual - truth|.
A window gap under 1e-6 fails the generator: change the seed, not the condition.
Usage: python tests/golden/gen_correct_logr.py"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, HERE)

import correctlogrsim  # noqa: E402
import gen_cli  # noqa: E402

ARGV = ["--tumor_logr_file", "logr.txt", "--gc_content_file", "gc.txt", "--replication_timing_file", "rt.txt",
        "--tumor_logr_correction_output_file", "out_LogR_Correction.txt", "--sample_name", "TUM"]
OUTPUT = "out_LogR_Correction.txt"
SCENARIOS = [
    dict(name="default", spec=dict(seed=3, G=18, T=12, extra=40, shuffle=True,
                                   chroms=[("chr1", 1100), ("chr2", 800), ("chr3", 500), ("chr1", 150), ("chrX", 450)])),
    dict(name="repeats", spec=dict(seed=8, G=18, T=12, extra=5, shuffle=False, repeats=12, chroms=[("chr1", 300), ("chr7", 250)])),
    dict(name="constant_column", spec=dict(seed=13, G=18, T=12, extra=5, shuffle=True, constant_gc=3, chroms=[("chr2", 400), ("chr5", 350)])),
    dict(name="narrow", spec=dict(seed=21, G=8, T=1, extra=3, shuffle=True, chroms=[("chr1", 300), ("chr4", 200)])),
    dict(name="missing_key", spec=dict(seed=34, G=18, T=12, extra=2, shuffle=True, missing=1, chroms=[("chr1", 60), ("chr3", 40)])),
]

CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
sys.argv = ["correct_logr"] + sys.argv[2:]
import numpy as np
import mpmath as mp
from sklearn.linear_model import LinearRegression
seen = dict(rows=None, cols=None, gaps=None, rank=None, truth=None, ref_err=None)
cap = dict(cc=[])
fit0, cc0 = LinearRegression.fit, np.corrcoef
def fit(self, X, y, *a, **k):
    cap["X"], cap["y"] = np.array(X, dtype=np.float64), np.array(y, dtype=np.float64).ravel()
    r = fit0(self, X, y, *a, **k)
    seen["rank"] = int(self.rank_)
    return r
def corrcoef(*a, **k):
    r = cc0(*a, **k)
    cap["cc"].append(np.abs(r)[0, 1:].copy())
    return r
LinearRegression.fit, np.corrcoef = fit, corrcoef
import correct_logr as m
m.main()
LinearRegression.fit, np.corrcoef = fit0, cc0

def choice(window, offset):
    at = int(np.argmax(window))
    if len(window) < 2 or np.isnan(window).any():
        return at + offset, None
    top = np.sort(window)[::-1]
    return at + offset, float((top[0] - top[1]) / top[0])
gc, rt = cap["cc"]
picks = [choice(gc[:6], 0), choice(gc[7:12], 7), choice(rt, 0)]
seen["cols"], seen["gaps"] = [p[0] for p in picks], [p[1] for p in picks]
seen["corr_gc"], seen["corr_rt"] = [repr(float(v)) for v in gc], [repr(float(v)) for v in rt]

mp.mp.prec = 200
X, y = cap["X"], cap["y"]
N, P = X.shape
seen["rows"] = N
xs = [[mp.mpf(float(v)) for v in row] for row in X]
ys = [mp.mpf(float(v)) for v in y]
xm = [mp.fsum(row[c] for row in xs) / N for c in range(P)]
ym = mp.fsum(ys) / N
xc = [[row[c] - xm[c] for c in range(P)] for row in xs]
yc = [v - ym for v in ys]
G, b = mp.matrix(P, P), mp.matrix(P, 1)
for r in range(P):
    b[r] = mp.fsum(xc[i][r] * yc[i] for i in range(N))
    for c in range(r, P):
        G[r, c] = G[c, r] = mp.fsum(xc[i][r] * xc[i][c] for i in range(N))
E, Q = mp.eigsy(G)
kept = [k for k in range(P) if E[k] > mp.mpf("1e-12") * max(E)]
seen["kept_eigenvalues"] = len(kept)
beta = mp.matrix(P, 1)
for k in kept:
    s = mp.fsum(Q[r, k] * b[r] for r in range(P)) / E[k]
    for r in range(P):
        beta[r] += Q[r, k] * s
truth = [yc[i] - mp.fsum(xc[i][r] * beta[r] for r in range(P)) for i in range(N)]
seen["truth"] = [mp.nstr(t, 25) for t in truth]
out = [float(ln.split("\t")[2]) for ln in open(sys.argv[sys.argv.index("--tumor_logr_correction_output_file") + 1]).read().split("\n")[1:] if ln]
seen["ref_err"] = repr(float(max(abs(mp.mpf(o) - t) for o, t in zip(out, truth))))
json.dump(seen, open("seen.json", "w"))
"""


def run_ref(d):
    return subprocess.run([sys.executable, "-W", "ignore", "-c", CHILD, os.path.join(REF, "src", "verdict")] + ARGV, cwd=d, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True)


def main():
    assert os.path.isdir(REF)
    tmp = tempfile.mkdtemp(prefix="gen_correct_logr_")
    out = []
    for sc in SCENARIOS:
        d = os.path.join(tmp, sc["name"])
        os.makedirs(d)
        files = correctlogrsim.tables(sc["spec"])
        for k, v in files.items():
            open(os.path.join(d, k), "w").write(v)
        p = run_ref(d)
        rec = dict(name=sc["name"], argv=ARGV, spec=sc["spec"], inputs_sha256=correctlogrsim.digest(files), returncode=p.returncode)
        if sc["name"] == "missing_key":
            last = p.stderr.strip().split("\n")[-1]
            assert p.returncode != 0 and last.startswith("KeyError: (") and not os.path.exists(os.path.join(d, OUTPUT)), (p.returncode, last)
            rec.update(output=None, seen=None, error=last, missing=list(eval(last[len("KeyError: "):])))
            print(sc["name"], p.returncode, last, flush=True)
        else:
            assert p.returncode == 0, p.stderr[-3000:]
            seen = json.load(open(os.path.join(d, "seen.json")))
            text = open(os.path.join(d, OUTPUT)).read()
            print(sc["name"], len(text), {k: v for k, v in seen.items() if k not in ("truth", "corr_gc", "corr_rt")}, flush=True)
            assert all(g is None or g >= 1e-6 for g in seen["gaps"]), seen["gaps"]
            assert seen["rank"] == 12 and seen["kept_eigenvalues"] == 12 and len(seen["truth"]) == seen["rows"] == text.count("\n") - 1
            if sc["name"] == "default":
                names = [c[0] for c in sc["spec"]["chroms"]]
                assert 2500 <= seen["rows"] <= 3500 and len(set(names)) >= 3 and all(g is not None for g in seen["gaps"])
            elif sc["name"] == "repeats":
                assert seen["rows"] == sum(c[1] for c in sc["spec"]["chroms"])        # the repeated logR keys kept their first place only
                assert all(files[k].count("\n") - 1 > seen["rows"] for k in files)
            elif sc["name"] == "constant_column":
                assert seen["corr_gc"][2] == "nan" and seen["cols"][0] == 2 and seen["gaps"][0] is None
            elif sc["name"] == "narrow":
                assert seen["cols"][1] == 7 and seen["cols"][2] == 0 and len(seen["corr_gc"]) == 8 and len(seen["corr_rt"]) == 1
            rec.update(output=text, seen=seen)
        out.append(rec)
    gen_cli.dump_json_gz("correct_logr.json.gz", dict(scenarios=out))
    shutil.rmtree(tmp, ignore_errors=True)
    print("wrote correct_logr.json.gz", os.path.getsize(os.path.join(HERE, "correct_logr.json.gz")), "bytes")


if __name__ == "__main__":
    main()
