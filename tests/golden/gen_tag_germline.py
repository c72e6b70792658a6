#!/usr/bin/env python3
"""The reference's tag_germline_variant (the last step of its Verdict chain, src/cna_germline_tagging.py:157-197), run from /root/reference
on the files of tagsim.py (needs the reference checkout, scipy, and this package built) -> tag_germline.json.gz.  Stored, data only: the
specs and seeds of the inputs, a SHA-256 of each input set, the argv lists (relative paths, run from the scenario's directory), every
output file's text, what the child printed and what it observed; a table of the binomial tests it ran with their exact values; the seven
command lines of the reference's driver for one set of options.

The reference's module does `from numpy import *`, and numpy 2 has round, max and min in its __all__ again: round(depth * frequency)
becomes a float that scipy rejects, max(P_G1, P_G2) would read P_G2 as an axis.  The module was written against the builtins, so the
child imports it from the checkout as it is and then puts the three builtins back into the module's namespace.  Nothing else is touched.

  * `default`: purity 0.4; segments of the classes (1,1), (2,0), (2,1), (3,1), (3,2), (0,0) and (6,1), in a file order that is not sorted,
    two of them overlapping so that the first in file order is not the first by start; a contig without a segment; calls on every
    segment's start and end; non-PASS rows, one ending in blanks; a repeated (contig, position); depths 8 - 300 and a few up to 3000;
    a test for which scipy returns 0.0 exactly.
  * `low_purity`: purity 0.25, the other side of `0.2 < p` together with `p >= 0.3`.
  * `high_purity`: purity 0.61: the warning, no output.   * `missing_cna`: no segment file: the warning, no output.
  * `gz`: 40 random rows, gzip-compressed, `in.vcf.gz`.
  * `commands`: the strings of the reference's seven *_command functions for one Namespace.

The child wraps binomtest and follows tag_germline_variant's frame line by line: which `SG_status =` lines ran, how often the two nan
branches, and at the head of the decision tree every quantity that decides.  The generator then fails (change the seed, not the
condition) when in `default` a `SG_status =` line other than 'unknown' never ran or a nan branch was not taken; when for any PASS call a
p-value lies within 1e-9 (relative) of 0.01, 1e-10 or 1e-4, the log-odds within 1e-9 of +-2 or +-5, or the AF within 1e-9 (relative) of
min_soma_EAF / 1.5 or min_germ_EAF / 2.0; and when on the far side of any test a term lies within 1e-9 (relative) of pmf(k) * (1 + 1e-7).
The error table: up to 600 of the distinct tests with n <= 400, in the order they ran: k, n, p (float.hex), scipy's p-value and the exact
one (fractions.Fraction, the same inclusion rule, as the nearest double); E_ref = scipy's largest relative error over the entries whose
exact value is >= 1e-14, E_ours = that of cto_binom_two_sided on the host path.
Usage: python tests/golden/gen_tag_germline.py"""
import gzip
import json
import math
import os
import shutil
import subprocess
import sys
import tempfile
from fractions import Fraction

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import gen_cli  # noqa: E402
import tagsim  # noqa: E402

ARGV = ["--input_vcf_fn", "in.vcf", "--output_fn", "out.vcf", "--tumor_purity_ploidy_output_file", "purity.txt", "--tumor_cna_output_file", "cna.txt"]
CONTIGS = [("chr1", 12000000), ("chr2", 12000000), ("chr3", 12000000), ("chr4", 12000000)]
SEGMENTS = [("chr1", 5000000, 9000000, 2, 1, False), ("chr1", 4000000, 6000000, 1, 1, False), ("chr1", 100000, 3500000, 2, 0, False),
            ("chr2", 1000000, 4000000, 3, 1, True), ("chr2", 4000001, 8000000, 3, 2, False), ("chr3", 2000000, 5000000, 0, 0, False),
            ("chr3", 6000000, 9000000, 6, 1, True), ("chr2", 8500000, 11000000, 1, 1, False)]
TARGETED = [(1, 300, "0.0800"), (2, 300, "0.1000"), (1, 300, "0.3000"), (1, 300, "0.4200"), (6, 300, "0.2400"), (1, 2500, "0.9000"), (5, 50, "0.0040"),
            (5, 80, "0.5000"), (7, 101, "0.4950")]
COMMON = dict(contigs=CONTIGS, segments=SEGMENTS, edges=True, gz=False, omit=[])
SCENARIOS = [
    dict(name="default", argv=ARGV, spec=dict(COMMON, seed=1, purity=0.4, rows=360, deep=6, targeted=TARGETED)),
    dict(name="low_purity", argv=ARGV, spec=dict(COMMON, seed=2, purity=0.25, rows=160, deep=2, targeted=TARGETED[:5])),
    dict(name="high_purity", argv=ARGV, spec=dict(COMMON, seed=3, purity=0.61, rows=30, deep=0, targeted=[])),
    dict(name="missing_cna", argv=ARGV, spec=dict(COMMON, seed=4, purity=0.4, rows=30, deep=0, targeted=[], omit=["cna.txt"])),
    dict(name="gz", argv=["--input_vcf_fn", "in.vcf.gz"] + ARGV[2:], spec=dict(COMMON, seed=5, purity=0.4, rows=37, deep=0, targeted=[], edges=False, gz=True)),
]
OPTIONS = dict(python="python3", verdict="/opt/verdict", parallel="parallel", threads=8, allele_counter="/opt/ac", tumor_bam_fn="tumor.bam", normal_bam_fn=None,
               cna_resource_dir="res", output_dir="out", tumor_sample_name="TUM", normal_sample_name="normal", contig_fn="contigs.txt", input_vcf_fn="in.vcf",
               output_fn="out/tagged.vcf", is_indel=False, platform="ont", tumor_purity=None)
CONTIG_FILE = "chr1\nchr2\nchrM\nchrX\nchrUn_KI270302v1\nchr21\n"

CHILD = r"""
import builtins, json, linecache, re, sys
sys.path.insert(0, sys.argv[1])
sys.argv = ["tag_germline_variant"] + sys.argv[2:]
import tag_germline_variant as m
m.round, m.max, m.min = builtins.round, builtins.max, builtins.min      # what the module was written against (numpy 2 exports its own again)
tests = []
real = m.binomtest
def spy(k, n, p, *a, **kw):
    r = real(k, n, p, *a, **kw)
    tests.append([int(k), int(n), float(p).hex(), float(r.pvalue)])
    return r
m.binomtest = spy
code = m.tag_germline_variant.__code__
src = linecache.getlines(code.co_filename)
status = {i + 1: re.search(r"SG_status = '([^']*)'", ln).group(1) for i, ln in enumerate(src) if "SG_status = '" in ln}
nan_s2 = [i + 1 for i, ln in enumerate(src) if ln.strip() == "AF_S2 = P_S2 = nan"]
nan_all = [i + 1 for i, ln in enumerate(src) if ln.strip() == "AF_G2 = AF_S2 = P_G2 = P_S2 = nan"]
head = [i + 1 for i, ln in enumerate(src) if "if frequency < 0.05 and 0.2 < p < 0.6:" in ln]
assert len(status) == 14 and len(nan_s2) == 1 and len(nan_all) == 1 and len(head) == 1, (status, nan_s2, nan_all, head)
seen = dict(status_lines={str(k): [v, 0] for k, v in status.items()}, nan_s2=0, nan_all=0, calls=[])
def local(frame, event, arg):
    if event == "line":
        ln = frame.f_lineno
        if ln in status:
            seen["status_lines"][str(ln)][1] += 1
        elif ln == nan_s2[0]:
            seen["nan_s2"] += 1
        elif ln == nan_all[0]:
            seen["nan_all"] += 1
        elif ln == head[0]:
            L = frame.f_locals
            seen["calls"].append(dict(ctg=L["ctg_name"], pos=L["pos"], seg=L["i"], n=L["depth"], f=float(L["frequency"]), logodds=float(L["logodds"]),
                                      mpg=float(L["max_prob_germline"]), mps=float(L["max_prob_somatic"]),
                                      AF=[float(L[k]) for k in ("AF_G1", "AF_S1", "AF_G2", "AF_S2")], P=[float(L[k]) for k in ("P_G1", "P_S1", "P_G2", "P_S2")]))
    return local
def tracer(frame, event, arg):
    return local if frame.f_code is code else None
sys.settrace(tracer)
m.main()
sys.settrace(None)
seen["tests"] = tests
print("SEEN " + json.dumps(seen))
"""

COMMANDS_CHILD = r"""
import argparse, json, sys
sys.path.insert(0, sys.argv[1])
import cna_germline_tagging as m
a = argparse.Namespace(**json.loads(sys.argv[2]))
print("SEEN " + json.dumps([m.tumor_allele_counter_command(a), m.get_logr_baf_command(a), m.correct_logr_command(a), m.predict_germline_genotypes_command(a),
                            m.create_aspcf_command(a), m.create_verdict_run_ascat_command(a), m.tag_germline_variant(a)]))
"""


def run_child(child, d, argv):
    p = subprocess.run([sys.executable, "-W", "ignore", "-c", child] + argv, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, (argv, p.stderr[-3000:])
    lines = p.stdout.split("\n")
    seen = [ln for ln in lines if ln.startswith("SEEN ")][-1]
    return json.loads(seen[5:]), "".join(ln + "\n" for ln in lines if ln and not ln.startswith("SEEN "))


def output_text(d, fn):
    """the output as text, whether or not a bgzip on this host compressed it afterwards"""
    if os.path.exists(os.path.join(d, fn)):
        return open(os.path.join(d, fn)).read()
    if os.path.exists(os.path.join(d, fn + ".gz")):
        return gzip.open(os.path.join(d, fn + ".gz"), "rt").read()
    return None


def away(x, t, what, call):
    assert abs(x - t) > 1e-9 * abs(t), (what, x, t, call)


def check_gaps(calls):
    for c in calls:
        for x in (c["mpg"], c["mps"]):
            for t in (0.01, 1e-10, 1e-4):
                away(x, t, "p-value", c)
        for t in (2.0, -2.0, 5.0, -5.0):
            assert not abs(c["logodds"] - t) <= 1e-9, ("log-odds", c)
        g1, s1, g2, s2 = c["AF"]
        away(c["f"], (s2 if s2 < s1 else s1) / 1.5, "min_soma_EAF / 1.5", c)
        away(c["f"], (g2 if g2 < g1 else g1) / 2.0, "min_germ_EAF / 2.0", c)


def check_far_side(tests):
    import numpy as np
    from scipy.stats import binom
    for k, n, ph, _ in tests:
        p = float.fromhex(ph)
        if p in (0.0, 1.0) or k == p * n:
            continue
        thr = binom.pmf(k, n, p) * (1 + 1e-7)
        if thr < 1e-280:
            continue
        far = np.arange(math.ceil(p * n), n + 1) if k < p * n else np.arange(0, math.floor(p * n) + 1)
        pm = binom.pmf(far, n, p)
        assert (np.abs(pm / thr - 1) > 1e-9).all(), ("far side", k, n, p)


def exact_pvalue(k, n, p):
    P = Fraction(p)
    Q = 1 - P
    pm, c = [], 1
    for i in range(n + 1):
        pm.append(c * P ** i * Q ** (n - i))
        c = c * (n - i) // (i + 1)
    pn = p * n
    if k == pn:
        return Fraction(1)
    thr = pm[k] * Fraction(1 + 1e-7)
    if k < pn:
        s = sum(pm[:k + 1]) + sum(x for i, x in enumerate(pm) if i >= math.ceil(pn) and x <= thr)
    else:
        s = sum(pm[k:]) + sum(x for i, x in enumerate(pm) if i <= math.floor(pn) and x <= thr)
    return min(Fraction(1), s)


def error_table(tests):
    from clairs_to_amd.tag_germline_variant import binom_two_sided
    entries, known = [], set()
    for k, n, ph, pv in tests:
        if n <= 400 and (k, n, ph) not in known and len(entries) < 600:
            known.add((k, n, ph))
            entries.append([k, n, ph, pv])
    ours = binom_two_sided([e[0] for e in entries], [e[1] for e in entries], [float.fromhex(e[2]) for e in entries], "host")
    e_ref = e_ours = Fraction(0)
    for e, o in zip(entries, ours):
        x = exact_pvalue(e[0], e[1], float.fromhex(e[2]))
        e.append(float(x))
        if x >= Fraction(1e-14):
            e_ref = max(e_ref, abs(Fraction(e[3]) - x) / x)
            e_ours = max(e_ours, abs(Fraction(float(o)) - x) / x)
        else:
            assert o < 1e-12, (e, o)
    return entries, float(e_ref), float(e_ours)


def main():
    assert os.path.isdir(REF)
    tmp = tempfile.mkdtemp(prefix="gen_tag_germline_")
    out, all_tests = [], []
    for sc in SCENARIOS:
        d = os.path.join(tmp, sc["name"])
        os.makedirs(d)
        built = tagsim.files(sc["spec"])
        tagsim.write(d, built)
        seen, printed = run_child(CHILD, d, [os.path.join(REF, "src", "verdict")] + sc["argv"])
        text = output_text(d, "out.vcf")
        outputs = {} if text is None else {"out.vcf": text}
        calls, tests = seen.pop("calls"), seen.pop("tests")
        check_gaps(calls)
        check_far_side(tests)
        all_tests += tests
        vcf = gzip.decompress(built["in.vcf.gz"]).decode() if "in.vcf.gz" in built else built["in.vcf"]
        body = [ln for ln in vcf.split("\n") if ln and ln[0] != "#"]
        keys = {}
        for ln in body:
            keys[tuple(ln.split("\t")[:2])] = ln.split()[6]
        seen.update(pass_calls=sum(v == "PASS" for v in keys.values()) if outputs else 0, calls_with_segment=len(calls), tests=len(tests),
                    zeros_from_scipy=sum(t[3] == 0.0 and float.fromhex(t[2]) not in (0.0, 1.0) for t in tests), rows=len(body), keys=len(keys),
                    deepest=max([c["n"] for c in calls], default=0), overlap_first=sum(c["seg"] == 0 and 5000000 <= c["pos"] <= 6000000 for c in calls),
                    on_an_edge=sum(any(s[0] == c["ctg"] and c["pos"] in (s[1], s[2]) for s in SEGMENTS) for c in calls))
        print(sc["name"], {k: len(v) for k, v in outputs.items()}, {k: v for k, v in seen.items() if k != "status_lines"}, repr(printed), flush=True)
        print("   ", {v[0] + "@" + k: v[1] for k, v in seen["status_lines"].items()}, flush=True)
        if sc["name"] == "default":
            assert all(v[1] >= 1 for v in seen["status_lines"].values() if v[0] != "unknown"), seen["status_lines"]
            assert seen["nan_s2"] >= 1 and seen["nan_all"] >= 1 and seen["zeros_from_scipy"] >= 1 and seen["overlap_first"] >= 1, seen
            assert seen["keys"] == seen["rows"] - 1 and seen["deepest"] > 1000 and seen["on_an_edge"] >= 2 * len(SEGMENTS) - 2 and printed == "", seen
            assert 380 <= seen["rows"] <= 420 and any(ln.endswith(" ") and "LowQual" in ln for ln in body)
            assert any(c["f"] < 0.05 for c in calls) and any(c["f"] > 0.95 for c in calls) and min(c["n"] for c in calls) <= 12
            assert seen["pass_calls"] > seen["calls_with_segment"] and any(ln.startswith("chr4\t") and "PASS" in ln for ln in body)
        elif sc["name"] == "low_purity":
            assert len(outputs) == 1 and seen["calls_with_segment"] > 50, seen
        elif sc["name"] in ("high_purity", "missing_cna"):
            assert not outputs and seen["tests"] == 0 and printed.startswith("[WARNING] "), (seen, printed)
        else:
            assert len(outputs) == 1 and seen["rows"] == 40 and seen["calls_with_segment"] >= 5, seen
        out.append(dict(name=sc["name"], argv=sc["argv"], spec=sc["spec"], inputs_sha256=tagsim.digest(built), outputs=outputs, printed=printed, seen=seen))

    open(os.path.join(tmp, "contigs.txt"), "w").write(CONTIG_FILE)
    strings, _ = run_child(COMMANDS_CHILD, tmp, [os.path.join(REF, "src"), json.dumps(OPTIONS)])
    assert len(strings) == 7
    entries, e_ref, e_ours = error_table(all_tests)
    summary = dict(entries=len(entries), entries_at_least_1e_14=sum(e[4] >= 1e-14 for e in entries), E_ref=e_ref, E_ours=e_ours)
    print("error table", summary)
    assert e_ours <= e_ref and len(entries) >= 300, summary
    gen_cli.dump_json_gz("tag_germline.json.gz", dict(scenarios=out, commands=dict(options=OPTIONS, contig_file=CONTIG_FILE, strings=strings),
                                                      error_table=dict(columns=["k", "n", "p", "scipy", "exact"], entries=entries, summary=summary)))
    shutil.rmtree(tmp, ignore_errors=True)
    size = os.path.getsize(os.path.join(HERE, "tag_germline.json.gz"))
    print("wrote tag_germline.json.gz", size, "bytes")
    assert size < os.path.getsize(os.path.join(HERE, "region2k.json.gz"))


if __name__ == "__main__":
    main()
