"""nonsomatic_tagging with the panel-of-normals scan on the device (csrc/pon.hip) against the reference (tests/golden/nonsomatic.json.gz):
every scenario's argv through the dispatch of `python -m clairs_to_amd nonsomatic_tagging`, output files and stdout byte for byte; and a seeded PoN of
600 000 records (BGZF with and without a .tbi, blocks and slabs cut inside lines) against a short restatement of the matching rule."""
import base64
import io
import os
import random
from contextlib import redirect_stdout

import numpy as np
import pytest

from conftest import load_json_gz
from ponutil import write_bgzf_vcf

pytestmark = pytest.mark.gpu


def materialise(d, files):
    for rel, b64 in files.items():
        p = os.path.join(d, rel)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "wb") as f:
            f.write(base64.b64decode(b64))


@pytest.mark.parametrize("name", ["ctg_four_kinds", "all_contigs", "options", "odd_lines", "aggregate"])
def test_scenario_byte_for_byte(name, tmp_path, monkeypatch):
    sc = next(s for s in load_json_gz("nonsomatic.json.gz")["scenarios"] if s["name"] == name)
    from clairs_to_amd.__main__ import dispatch
    d = str(tmp_path)
    materialise(d, sc["inputs"])
    monkeypatch.setenv("CTO_PON_SLAB", str(1 << 17))         # the smallest slab: lines and blocks cross slabs
    monkeypatch.chdir(d)
    for run in sc["runs"]:                                   # `python -m clairs_to_amd nonsomatic_tagging <argv>`, in this process
        buf, rc = io.StringIO(), 0
        with redirect_stdout(buf):
            try:
                dispatch("nonsomatic_tagging", list(run["argv"]))
            except SystemExit as e:
                rc = e.code if isinstance(e.code, int) else 1
        assert (rc == 0) == (run["returncode"] == 0), run["argv"]
        if run["returncode"] == 0:
            assert buf.getvalue() == run["stdout"], run["argv"]
    got = {}
    for b, _, fs in os.walk(d):
        for f in fs:
            rel = os.path.relpath(os.path.join(b, f), d)
            if rel not in sc["inputs"]:
                got[rel] = open(os.path.join(b, f), "rb").read()
    assert sorted(got) == sorted(sc["outputs"])
    for rel, b64 in sc["outputs"].items():
        assert got[rel] == base64.b64decode(b64), rel


def test_whole_run_step3_and_step7(tmp_path, monkeypatch):
    """the commands `run_clairs_to --panel_of_normals ...` builds for STEP 3 / STEP 7 (one invocation per contig, the sort_vcf merges, the
    sample summaries), in order, on the ont_whole run's pileup VCFs: every file the reference wrote and its summary lines, byte for byte"""
    from clairs_to_amd.__main__ import dispatch
    wr = load_json_gz("nonsomatic.json.gz")["whole_run"]
    T, W = tmp_path / "t", tmp_path / "w"
    materialise(str(T), wr["scratch_files"])
    materialise(str(W), {k: v for k, v in wr["scratch_files"].items() if k.startswith("pon/")})     # the PoNs are given relative to the run
    (W / "tmp" / "vcf_output").mkdir(parents=True)
    fill = lambda s: s.replace("@W@", str(W)).replace("@T@", str(T))                                 # noqa: E731
    (W / "tmp" / "CONTIGS").write_text(fill(wr["contigs"]))
    for name, text in wr["pileup"].items():
        (W / "tmp" / "vcf_output" / name).write_text(text)
    monkeypatch.chdir(W)
    for run in wr["runs"]:
        buf = io.StringIO()
        with redirect_stdout(buf):
            dispatch(run["submodule"], [fill(t) for t in run["argv"]])
        if run["submodule"] == "nonsomatic_tagging":
            assert buf.getvalue() == fill(run["stdout"]), run["argv"]
    for name, text in wr["outputs"].items():
        assert (W / "tmp" / "vcf_output" / name).read_text() == fill(text), name


def restated_hits(text, calls, only, require_allele):
    """the matching rule of src/nonsomatic_tagging.py for well-formed tab-separated lines"""
    by = {(c, p): i for i, (c, p, _, _) in enumerate(calls)}
    hit = np.zeros(len(calls), np.uint8)
    for line in text.split("\n"):
        if not line or line[0] == "#":
            continue
        f = line.split("\t", 5)
        if only is not None and f[0] != only:
            continue
        i = by.get((f[0], int(f[1])))
        if i is None:
            continue
        if not require_allele or (calls[i][2] == f[3] and calls[i][3] in f[4].split(",")):
            hit[i] = 1
    return hit


def test_synthetic_pon_against_the_rule(tmp_path, monkeypatch):
    import torch
    from clairs_to_amd.nonsomatic_tagging import PonScanner
    rng = random.Random(7)
    contigs = ["chr%d" % i for i in (1, 2, 3, 4)]
    lines, calls = ["##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"], []
    for c in contigs:
        pos = 0
        for _ in range(150000):
            pos += rng.randint(1, 40)
            ref, alt = rng.choice("ACGT"), rng.choice(["A", "C", "G", "T", "AC", "G,T"])
            lines.append("%s\t%d\t.\t%s\t%s\t50\tPASS\tAF=0.%d\n" % (c, pos, ref, alt, rng.randint(1, 99999)))
            if rng.random() < 0.01:
                calls.append((c, pos, ref if rng.random() < 0.7 else "T", alt.split(",")[-1] if rng.random() < 0.7 else "C"))
    text = "".join(lines)
    path = str(tmp_path / "pon.vcf.gz")
    write_bgzf_vcf(path, text.encode(), with_tbi=True)
    sets = {}
    for c, p, r, a in calls:
        sets.setdefault(c, {})[p] = dict(ref=r, alt=a)
    monkeypatch.setenv("CTO_PON_SLAB", str(1 << 20))
    torch.cuda.init()
    sc = PonScanner(sets)
    try:
        for require in (True, False):
            want = restated_hits(text, calls, None, require)
            got, st, host = sc.match(path, None, require)
            assert not host and st.used_tbi == 0 and st.kind == 1 and st.records == 600000
            assert got == {(c, p) for (c, p, _, _), h in zip(calls, want) if h}
        only = {"chr3": sets["chr3"]}
        sc.close()
        sc = PonScanner(only)
        calls3 = [x for x in calls if x[0] == "chr3"]
        want = restated_hits(text, calls3, "chr3", True)
        got, st_tbi, _ = sc.match(path, "chr3", True)
        assert st_tbi.used_tbi == 1 and got == {(c, p) for (c, p, _, _), h in zip(calls3, want) if h}
        assert st_tbi.records == 150000
        os.rename(path + ".tbi", path + ".tbi.off")
        got2, st_full, _ = sc.match(path, "chr3", True)
        assert st_full.used_tbi == 0 and got2 == got
        assert st_tbi.bytes_read < 0.4 * st_full.bytes_read          # the index cut the bytes read to about a quarter
    finally:
        sc.close()
