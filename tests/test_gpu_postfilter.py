"""postfilter_variants with the per-call window rules on the device (csrc/postfilter.hip) against the reference (tests/golden/postfilter.json.gz):
every scenario's argv through the dispatch of `python -m clairs_to_amd postfilter_variants` with the samtools stand-in on PATH - output VCF,
PF_INFO_* and stdout byte for byte, the per-position form's line, the same VCF however the calls are cut into jobs and whatever the thread
count; and, on windows freshly seeded every run, the integers of cto_postfilter_windows against a short plain-Python restatement of
src/postfilter_variants.py:147-179, :239-260, :286-350, :376-445, through the kernel and through the host path of the same call."""
import io
import os
import random
import stat
from collections import Counter
from contextlib import redirect_stdout

import numpy as np
import pytest

import pfsim
from conftest import load_json_gz

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load_json_gz("postfilter.json.gz")


def set_up(d, spec, monkeypatch):
    files = pfsim.scenario_files(spec)
    for k, v in files.items():
        open(os.path.join(d, k), "w").write(v)
    open(os.path.join(d, "t.bam"), "w").close()
    fn = os.path.join(d, "samtools")
    open(fn, "w").write(pfsim.SHIM_SAMTOOLS)
    os.chmod(fn, os.stat(fn).st_mode | stat.S_IEXEC)
    monkeypatch.setenv("PATH", d + os.pathsep + os.environ["PATH"])
    monkeypatch.chdir(d)
    return files


def run_mirror(argv):
    from clairs_to_amd.__main__ import dispatch
    buf = io.StringIO()
    with redirect_stdout(buf):
        dispatch("postfilter_variants", list(argv))
    return buf.getvalue()


def outputs_of(argv):
    out_fn = argv[argv.index("--output_vcf_fn") + 1]
    work = argv[argv.index("--output_dir") + 1]
    info = sorted(f for f in os.listdir(work) if f.startswith("PF_INFO")) if os.path.isdir(work) else []
    return dict(link=os.readlink(out_fn) if os.path.islink(out_fn) else None, out_vcf=None if os.path.islink(out_fn) else open(out_fn).read(),
                pf_info={f: open(os.path.join(work, f)).read() for f in info})


@pytest.mark.parametrize("name", ["main", "options", "odd"])
def test_scenario_byte_for_byte(golden, name, tmp_path, monkeypatch):
    sc = next(s for s in golden["scenarios"] if s["name"] == name)
    files = set_up(str(tmp_path), sc["spec"], monkeypatch)
    assert pfsim.digest(files) == sc["inputs_sha256"]
    assert len(sc["runs"]) >= 2
    for run in sc["runs"]:
        stdout = run_mirror(run["argv"])
        got = outputs_of(run["argv"])
        assert got["link"] == run["link"], run["name"]
        assert got["pf_info"] == run["pf_info"], run["name"]
        assert got["out_vcf"] == run["out_vcf"], run["name"]
        assert stdout == run["stdout"], run["name"]
        os.remove(run["argv"][run["argv"].index("--output_vcf_fn") + 1])
        if os.path.isdir("out"):
            os.rmdir("out")                                    # every run finds the output folder missing, as the reference's did
    assert len(sc["per_pos"]) >= 4
    for rec in sc["per_pos"]:                                  # the worker form: one call on the command line, one line on stdout
        assert run_mirror(rec["argv"]) == rec["stdout"], rec["argv"]


@pytest.mark.parametrize("cut", [("1", "1", "300"), ("3", "7", "50000"), ("1000", "12", "1000000")])
def test_job_cut_and_thread_count_do_not_matter(golden, cut, tmp_path, monkeypatch):
    sc = next(s for s in golden["scenarios"] if s["name"] == "main")
    set_up(str(tmp_path), sc["spec"], monkeypatch)
    for run in sc["runs"][:2]:
        argv = [t for t in run["argv"]]
        argv[argv.index("--threads") + 1] = cut[1]
        run_mirror(argv + ["--job_max_sites", cut[0], "--job_max_span", cut[2]])
        assert outputs_of(argv)["out_vcf"] == run["out_vcf"], (run["name"], cut)


# ------------------------------------------------------------------------------------------ the restatement
def parse_rows(text):
    rows = {}
    for row in text.splitlines(keepends=True):
        c = row.split("\t")
        if len(c) < 8:
            continue
        s, ents, st, en, i = c[4], [], set(), set(), 0
        while i < len(s):
            b = s[i]
            if b in "+-":
                i, n = i + 1, 0
                while s[i].isdigit():
                    n, i = n * 10 + int(s[i]), i + 1
                ents[-1][1] = b + s[i:i + n]
                i += n - 1
            elif b in "ACGTNacgtn#*":
                ents.append([b, ""])
            elif b == "^":
                i += 1
                st.add(len(ents) - 1)
            if b == "$":
                en.add(len(ents) - 1)
            i += 1
        names = c[7].split(",")
        for k, e in enumerate(ents):
            names[k] += "_1" if e[0] == "#" or e[0].islower() else "_0"
        rows[int(c[1])] = (names, [(e[0].upper(), e[1]) for e in ents], st if len(st) > len(en) else en)
    return rows


def restated_counts(rows, ref, lo, pos, rb, ab, fl):
    A, S, depth, fwd, rev, match, ins = set(), set(), 0, 0, 0, 0, 0
    cols = {p: rows[p] for p in range(max(pos - fl, 1), pos + fl + 1) if p in rows}
    for p, (names, ents, rse) in cols.items():
        if len(rse) >= len(ents) * 0.2:
            S |= {names[i] for i in rse}
        if p == pos:
            depth, fwd, rev = len(names), sum(n.endswith("0") for n in names), sum(n.endswith("1") for n in names)
            for n, (b, ind) in zip(names, ents):
                v = b + ind
                if (len(rb) == 1 == len(ab) and v == ab) or (len(rb) == 1 < len(ab) and "+" in v and v.replace("+", "").upper() == ab) or \
                        (len(rb) > 1 and len(ab) == 1 and len(ind) == len(rb) and "-" in ind):
                    A.add(n)
    for p, (names, ents, rse) in cols.items():
        if p == pos:
            continue
        d = dict(zip(names, ents))
        ins += sum(min(len(v[1]) - 1, 2 * fl) for v in d.values() if len(v[1]) > 3 and v[1][0] == "+")
        cnt = Counter((v[0] + v[1]).upper() for k, v in d.items() if k in A and (v[0] + v[1]).upper() != ref[p - lo] and (v[0] + v[1]).upper() not in "#*")
        if not cnt:
            continue
        tok, c = max(cnt.items(), key=lambda x: x[1])
        if c >= len(A) * 1.5 or c <= len(A) * 0.5 or sum((e[0] + e[1]).upper() == tok for e in ents) >= c * 1.5:
            continue
        match += 1
    a0, a1 = sum(n.endswith("0") for n in A), sum(n.endswith("1") for n in A)
    return [len(A), len(A & S), match, ins, depth, a0, fwd - a0, a1, rev - a1]


def test_fresh_windows_against_the_restatement():
    from clairs_to_amd.postfilter_variants import PackedJob, evaluate_windows
    seed = random.SystemRandom().randrange(1 << 30)
    print("seed", seed)
    rng = random.Random(seed)
    jobs, calls, want = [], [], []
    for j in range(3):
        fl = (100, 100, 37)[j]
        sim = pfsim.simulate(rng.randrange(1 << 30), depth=rng.choice((8, 30, 70)), odd=j == 1)
        cs = [c for c in sim["snv_calls"] + sim["indel_calls"] if c[0] < 5100]
        cs += [(rng.randrange(1, 5100), "A", "C") for _ in range(10)] + [(rng.randrange(1, 5100), "ACG", "A") for _ in range(5)]
        positions = sorted({p for c in cs for p in range(max(1, c[0] - fl - 3), c[0] + fl + 4)} - set(rng.sample(range(1, 5200), 80)))
        text = pfsim.pileup_text(sim, "c", positions)
        jobs.append(PackedJob(text, sim["ref"], 1, fl))
        rows = parse_rows(text)
        for c in cs:
            calls.append((j, c[0], c[1], c[2]))
            want.append(restated_counts(rows, sim["ref"], 1, c[0], c[1], c[2], fl))
    assert len(calls) > 150
    want = np.array(want, dtype=np.int64)
    assert (want[:, 0] > 0).sum() > 60 and (want[:, 1] > 0).sum() > 5 and (want[:, 2] > 0).sum() > 5 and (want[:, 3] > 0).sum() > 5
    got = evaluate_windows(jobs, calls)
    assert (got[:, 9] == 0).all()                              # every window fits the kernel
    bad = np.nonzero((got[:, :9] != want).any(axis=1))[0]
    assert bad.size == 0, (seed, [(calls[i], got[i].tolist(), want[i].tolist()) for i in bad[:5]])
    forced = evaluate_windows(jobs, calls, max_id_range=24)    # narrow bitsets: most windows go through the host path of the same call
    assert (forced[:, 9] == 1).sum() > 100
    assert (forced[:, :9] == want).all(), seed


def test_a_window_too_wide_for_the_bitsets_takes_the_host_path():
    from clairs_to_amd.postfilter_variants import PackedJob, evaluate_windows
    # (a ninth field, so that a row's last name carries no '\n' and 'early' is ONE key in its first row and in the window)
    row = lambda p, bases, names: "c\t%d\tN\t%d\t%s\t%s\t%s\t%s\t-\n" % (p, len(names), bases, "I" * len(names), "]" * len(names), ",".join(names))
    rows = [row(1, "A", ["early"])] + [row(1 + i, "A", ["f%d" % i]) for i in range(1, 9001)]
    late = ["l%d" % i for i in range(12)]
    for p in range(20000, 20041):
        alt = p in (20020, 20025, 20031)
        rows.append(row(p, ("T" if alt else "A") + "".join(("t" if alt and i % 2 else "a") for i in range(12)) + "$", ["early"] + late))
    text = "".join(rows)
    ref = "A" * 20200
    job = PackedJob(text, ref, 1, 100)
    calls = [(0, 20020, "A", "T"), (0, 20000, "A", "T"), (0, 5000, "A", "C")]
    got = evaluate_windows([job], calls)
    assert got[:, 9].tolist() == [1, 1, 0]                     # 'early' .. 'l11' span more than 8192 read ids
    parsed = parse_rows(text)
    for c, g in zip(calls, got):
        assert g[:9].tolist() == restated_counts(parsed, ref, 1, c[1], c[2], c[3], 100), c
    assert got[0, 0] == 7 and got[0, 2] == 2


def test_the_c_call_raises_without_a_device(tmp_path):
    """no CPU fallback: in a child process that sees no HIP device, packing still works (host code) and cto_postfilter_windows refuses"""
    import subprocess
    import sys
    from conftest import ROOT
    script = tmp_path / "no_device.py"
    script.write_text("import sys\nsys.path.insert(0, %r)\n"
                      "from clairs_to_amd._lib import CtoError\n"
                      "from clairs_to_amd.postfilter_variants import PackedJob, evaluate_windows\n"
                      "job = PackedJob('c\\t5\\tN\\t2\\tAt\\tII\\t]]\\ta,b\\t-\\n', 'ACGTACGTAC', 1, 100)\n"
                      "try:\n    evaluate_windows([job], [(0, 5, 'A', 'T')])\n    print('RAN')\n"
                      "except CtoError as e:\n    print('RAISED', e)\n" % ROOT)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    p = subprocess.run([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.startswith("RAISED") and "no HIP device" in p.stdout, p.stdout


def test_whole_run_step_4_2_and_8_2(golden, tmp_path, monkeypatch):
    """the postfilter_variants and postprocess_vcf command lines `run_clairs_to -p ilmn --dry_run` builds, in order, on realignment VCFs of
    two simulated contigs (no --ctg_name): stdout and every file the reference wrote, down to the post-processed snv.vcf / indel.vcf"""
    from clairs_to_amd.__main__ import dispatch
    wr = golden["whole_run"]
    t = str(tmp_path)
    w = os.path.join(t, "runs", "ilmn_whole_postfilter")
    files = pfsim.scenario_files(wr["spec"])
    assert pfsim.digest(files) == wr["inputs_sha256"]
    sub = lambda x: x.replace("@W@", w).replace("@T@", t)
    os.makedirs(os.path.join(w, "tmp", "vcf_output"))
    os.makedirs(os.path.join(t, "in"))
    open(os.path.join(t, "in", "ref.fa"), "w").write(files["ref.fa"])
    open(os.path.join(t, "in", "ref.fa.fai"), "w").write(files["ref.fa.fai"])
    open(os.path.join(t, "in", "t.bam"), "w").close()
    open(os.path.join(w, "mp.txt"), "w").write(files["mp.txt"])
    for rel, text in wr["run_files"].items():
        open(os.path.join(w, rel), "w").write(sub(text))
    for mode in ("snv", "indel"):
        open(os.path.join(w, "tmp", "vcf_output", "%s_pileup_realignment.vcf" % mode), "w").write(files["in_%s.vcf" % mode])
    bin_dir = os.path.join(t, "bin")
    os.makedirs(bin_dir)
    fn = os.path.join(bin_dir, "samtools")
    open(fn, "w").write(pfsim.SHIM_SAMTOOLS)
    os.chmod(fn, os.stat(fn).st_mode | stat.S_IEXEC)
    monkeypatch.setenv("PATH", bin_dir + os.pathsep + os.environ["PATH"])
    monkeypatch.chdir(w)
    before = {os.path.relpath(os.path.join(b, f), w) for b, _, fs in os.walk(w) for f in fs}
    assert [r["submodule"] for r in wr["runs"]].count("postfilter_variants") == 2 and [r["submodule"] for r in wr["runs"]].count("postprocess_vcf") == 2
    for run in wr["runs"]:
        buf = io.StringIO()
        with redirect_stdout(buf):
            dispatch(run["submodule"], [sub(a) for a in run["argv"]])
        assert buf.getvalue() == sub(run["stdout"]), run["argv"]
    got = {os.path.relpath(os.path.join(b, f), w) for b, _, fs in os.walk(w) for f in fs} - before
    assert got == set(wr["outputs"])
    for rel, rec in wr["outputs"].items():
        assert "text" in rec and open(os.path.join(w, rel)).read() == sub(rec["text"]), rel
    assert wr["outputs"]["snv.vcf"]["text"].count(";SB=") + wr["outputs"]["indel.vcf"]["text"].count(";SB=") >= 100
