"""tag_germline_variant (the last step of the reference's Verdict chain) and cna_germline_tagging (that chain's driver) against what the
reference wrote, printed and would have run on the same inputs (tests/golden/tag_germline.json.gz, written by
tests/golden/gen_tag_germline.py): every argv through the dispatch of `python -m clairs_to_amd`, byte for byte, through the host path of
cto_tag_germline; the test rule against exact rational arithmetic, held to the error scipy itself makes on the same tests; the segment,
fraction and test rules against values written out by hand; the failures; the driver's argument lists."""
import glob
import gzip
import math
import os
import re
import shlex
from fractions import Fraction

import numpy as np
import pytest

import tagsim
from conftest import ROOT, load_json_gz

SCENARIOS = ["default", "low_purity", "high_purity", "missing_cna", "gz"]
NAN = float("nan")
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def golden():
    return load_json_gz("tag_germline.json.gz")


def write_inputs(d, sc):
    built = tagsim.files(sc["spec"])
    assert tagsim.digest(built) == sc["inputs_sha256"]
    tagsim.write(d, built)
    return sorted(built)


def output_text(fn):
    """the output as text, whether or not a bgzip on this host compressed it afterwards"""
    if os.path.exists(fn):
        return open(fn).read()
    if os.path.exists(fn + ".gz"):
        return gzip.open(fn + ".gz", "rt").read()
    return None


def run_scenario(sc, where, capsys):
    """the scenario's argv in the current directory: its output and what it printed, compared; nothing else written"""
    from clairs_to_amd.__main__ import dispatch
    inputs = sorted(os.listdir("."))
    capsys.readouterr()
    dispatch("tag_germline_variant", list(sc["argv"]) + ["--where", where])
    assert capsys.readouterr().out == sc["printed"], sc["name"]
    if "out.vcf" in sc["outputs"]:
        assert output_text("out.vcf") == sc["outputs"]["out.vcf"], sc["name"]
        for fn in glob.glob("out.vcf*"):
            os.remove(fn)
    assert sorted(os.listdir(".")) == inputs, sc["name"]


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


def exact_test(k, n, p):
    """the two-sided p-value of scipy's rule in rational arithmetic"""
    P = Fraction(p)
    pm, c = [], 1
    for i in range(n + 1):
        pm.append(c * P ** i * (1 - P) ** (n - i))
        c = c * (n - i) // (i + 1)
    if k == p * n:
        return Fraction(1)
    thr = pm[k] * Fraction(1 + 1e-7)
    if k < p * n:
        return min(Fraction(1), sum(pm[:k + 1]) + sum(x for i, x in enumerate(pm) if i >= math.ceil(p * n) and x <= thr))
    return min(Fraction(1), sum(pm[k:]) + sum(x for i, x in enumerate(pm) if i <= math.floor(p * n) and x <= thr))


def close(got, want, rel=4 * 2.0 ** -52):
    """a handful of fp64 roundings apart at the most"""
    return abs(got - want) <= rel * want


def host_test(k, n, p):
    from clairs_to_amd.tag_germline_variant import binom_two_sided
    return float(binom_two_sided([k], [n], [p], "host")[0])


TABLE = dict(seg_chr=[0, 0, 1, 0], seg_start=[500, 100, 100, 100], seg_end=[900, 600, 200, 100], seg_nmaj=[2, 1, 2, 3], seg_nmin=[1, 1, 0, 1])


def host_calls(ctg, pos, depth, freq, purity=0.4, table=TABLE, stats=None, where="host"):
    from clairs_to_amd.tag_germline_variant import tag_calls
    return tag_calls(ctg, pos, depth, freq, table["seg_chr"], table["seg_start"], table["seg_end"], table["seg_nmaj"], table["seg_nmin"], purity, where, stats)


def test_both_names_are_submodules():
    from clairs_to_amd.__main__ import SUBMODULES
    assert "tag_germline_variant" in SUBMODULES and "cna_germline_tagging" in SUBMODULES


def test_no_file_of_the_package_imports_scipy():
    files = glob.glob(os.path.join(ROOT, "clairs_to_amd", "**", "*.py"), recursive=True)
    assert len(files) > 20
    for fn in files:
        assert not re.search(r"^\s*(import|from)\s+scipy\b", open(fn).read(), re.M), fn


def test_the_python_constant_is_the_header_s():
    header = open(os.path.join(ROOT, "include", "clairsto_amd.h")).read()
    assert int(re.search(r"#define CTO_TAG_WAVES_PER_GROUP\s+(\d+)", header).group(1)) == 4


def test_the_fixture_holds_what_the_issue_asks_for(golden):
    by_name = {sc["name"]: sc for sc in golden["scenarios"]}
    assert list(by_name) == SCENARIOS
    d = by_name["default"]
    seen = d["seen"]
    assert d["spec"]["purity"] == 0.4 and len(d["spec"]["contigs"]) == 4 and 380 <= seen["rows"] <= 420
    classes = {(s[3], s[4]) for s in d["spec"]["segments"]}
    assert {(1, 1), (2, 0), (2, 1), (3, 1), (3, 2), (0, 0)} <= classes
    assert {s[0] for s in d["spec"]["segments"]} < {c[0] for c in d["spec"]["contigs"]}            # a contig without a segment
    assert all(n >= 1 for what, n in seen["status_lines"].values() if what != "unknown") and len(seen["status_lines"]) == 14
    assert seen["nan_s2"] >= 1 and seen["nan_all"] >= 1 and seen["zeros_from_scipy"] >= 1 and seen["overlap_first"] >= 1
    assert seen["keys"] == seen["rows"] - 1 and seen["deepest"] > 1000 and seen["on_an_edge"] >= 14
    assert by_name["low_purity"]["spec"]["purity"] == 0.25 and by_name["high_purity"]["spec"]["purity"] == 0.61
    assert by_name["high_purity"]["outputs"] == {} and by_name["high_purity"]["printed"].startswith("[WARNING] Tumor purity estimation 0.61")
    assert by_name["missing_cna"]["outputs"] == {} and by_name["missing_cna"]["printed"].startswith("[WARNING] Verdict can not obtain")
    assert by_name["gz"]["argv"][1] == "in.vcf.gz" and by_name["gz"]["seen"]["rows"] == 40
    assert len(golden["commands"]["strings"]) == 7
    table = golden["error_table"]
    assert 300 <= len(table["entries"]) <= 600 and all(e[1] <= 400 for e in table["entries"])
    assert table["summary"]["E_ours"] <= table["summary"]["E_ref"]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "tag_germline.json.gz")) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "region2k.json.gz"))


@pytest.mark.parametrize("name", SCENARIOS)
def test_every_scenario_byte_for_byte_on_the_host_path(golden, name, tmp_path, monkeypatch, capsys):
    sc = next(s for s in golden["scenarios"] if s["name"] == name)
    write_inputs(str(tmp_path), sc)
    monkeypatch.chdir(tmp_path)
    run_scenario(sc, "host", capsys)


def test_the_counts_are_the_generator_s(golden, tmp_path, monkeypatch):
    from clairs_to_amd.tag_germline_variant import tag_germline_variant
    sc = golden["scenarios"][0]
    write_inputs(str(tmp_path), sc)
    monkeypatch.chdir(tmp_path)
    st = {}
    tag_germline_variant("in.vcf", "out.vcf", "purity.txt", "cna.txt", where="host", stats=st)
    assert st == dict(n_calls=sc["seen"]["pass_calls"], n_with_segment=sc["seen"]["calls_with_segment"], n_tests=sc["seen"]["tests"], host_path=1, kernel_ms=0.0)


def test_the_test_rule_is_within_scipy_s_own_error_of_the_exact_value(golden):
    """Entry by entry: where the exact value is at least 1e-14 our relative error is at most E_ref, the largest scipy makes on these same
    entries (no margin); elsewhere our value is below 1e-12.  The generator measured E_ref = 1.7e-14 and, for this rule, 3.5e-15."""
    from clairs_to_amd.tag_germline_variant import binom_two_sided
    table = golden["error_table"]
    entries = table["entries"]
    e_ref = table["summary"]["E_ref"]
    ours = binom_two_sided([e[0] for e in entries], [e[1] for e in entries], [float.fromhex(e[2]) for e in entries], "host")
    worst, worst_ref = Fraction(0), Fraction(0)
    for (k, n, p, from_scipy, exact), got in zip(entries, ours):
        if exact >= 1e-14:
            worst = max(worst, abs(Fraction(float(got)) - Fraction(exact)) / Fraction(exact))
            worst_ref = max(worst_ref, abs(Fraction(from_scipy) - Fraction(exact)) / Fraction(exact))
        else:
            assert got < 1e-12, (k, n, p, got)
    print("largest relative error: ours %.3g, scipy's %.3g (stored E_ref %.3g, E_ours %.3g)" % (worst, worst_ref, e_ref, table["summary"]["E_ours"]))
    assert 0 < e_ref < 1e-12 and abs(float(worst_ref) - e_ref) <= 0.02 * e_ref      # the table holds the exact values as the nearest doubles
    assert worst <= Fraction(e_ref), (float(worst), e_ref)


def test_the_segment_rule_is_the_first_in_file_order():
    #          row 0 holds 500..900, row 1 holds 100..600 on the same contig: 550 is in both and row 0 comes first; a sort would say row 1
    ctg = [0, 0, 0, 0, 0, 0, 1, 1, 2, 0, 0]
    pos = [550, 500, 900, 499, 100, 901, 100, 201, 150, 600, 601]
    seg, af, pv = host_calls(ctg, pos, [30] * len(ctg), [0.5] * len(ctg))
    assert seg.tolist() == [0, 0, 0, 1, 1, -1, 2, -1, -1, 0, 0]
    assert np.isnan(af[seg < 0]).all() and np.isnan(pv[seg < 0]).all() and not np.isnan(af[seg >= 0][:, :2]).any()
    st = {}
    seg, af, pv = host_calls([0], [100], [30], [0.5], table=dict(seg_chr=[0, 0], seg_start=[100, 100], seg_end=[100, 100], seg_nmaj=[3, 1], seg_nmin=[1, 1]), stats=st)
    assert seg.tolist() == [0] and st == dict(n_calls=1, n_with_segment=1, n_tests=4, host_path=1, kernel_ms=0.0)
    empty = dict(seg_chr=[], seg_start=[], seg_end=[], seg_nmaj=[], seg_nmin=[])
    seg, af, pv = host_calls([0, 1], [5, 6], [30, 30], [0.5, 0.5], table=empty, stats=st)
    assert seg.tolist() == [-1, -1] and np.isnan(af).all() and np.isnan(pv).all() and st["n_tests"] == 0 and st["n_with_segment"] == 0


def test_the_fraction_rule_and_its_two_nan_cases():
    p = 0.4
    den = lambda C: p * C + 2 * (1 - p) + EPS
    # row 0 (2,1): four fractions; row 1 (1,1): M == C - M, G2 and S2 are nan; row 2 (2,0): M becomes C, C - M == 0, S2 is nan
    seg, af, pv = host_calls([0, 0, 1], [700, 200, 150], [40, 40, 40], [0.3, 0.3, 0.3], purity=p)
    assert seg.tolist() == [0, 1, 2]
    assert same_bits(af[0], [(p * 1 + 1 * (1 - p)) / den(3), (p * 1 + 0 * (1 - p)) / den(3), (p * 2 + 1 * (1 - p)) / den(3), (p * 2 + 0 * (1 - p)) / den(3)])
    assert same_bits(af[1], [(p * 1 + 1 * (1 - p)) / den(2), (p * 1 + 0 * (1 - p)) / den(2), NAN, NAN]) and np.isnan(pv[1, 2:]).all()
    assert same_bits(af[2], [(p * 2 + 1 * (1 - p)) / den(2), (p * 2 + 0 * (1 - p)) / den(2), (p * 0 + 1 * (1 - p)) / den(2), NAN])
    assert np.isnan(pv[2, 3]) and not np.isnan(pv[2, :3]).any() and not np.isnan(pv[0]).any()
    # k = round(n * AF), half to even: 0.5 * 5 = 2.5 -> 2, 0.5 * 7 = 3.5 -> 4
    _, af, pv = host_calls([0, 0], [200, 200], [5, 7], [0.5, 0.5], purity=p)
    assert same_bits(pv[0, :2], [host_test(2, 5, af[0, 0]), host_test(2, 5, af[0, 1])])
    assert same_bits(pv[1, :2], [host_test(4, 7, af[1, 0]), host_test(4, 7, af[1, 1])])
    # the (0,0) segment: AF_S1 is 0, and the test against it is 1 when no read shows the allele and 0 otherwise
    zero = dict(seg_chr=[0], seg_start=[1], seg_end=[9], seg_nmaj=[0], seg_nmin=[0])
    _, af, pv = host_calls([0, 0], [5, 5], [50, 50], [0.004, 0.5], purity=p, table=zero)
    assert af[0, 1] == 0.0 and pv[:, 1].tolist() == [1.0, 0.0] and np.isnan(af[:, 2:]).all()


def test_the_test_rule_on_values_written_out_by_hand():
    assert [host_test(0, 7, 0.0), host_test(1, 7, 0.0), host_test(7, 7, 0.0)] == [1.0, 0.0, 0.0]           # p = 0
    assert [host_test(7, 7, 1.0), host_test(6, 7, 1.0), host_test(0, 7, 1.0)] == [1.0, 0.0, 0.0]           # p = 1
    assert host_test(5, 10, 0.5) == 1.0 and host_test(3, 12, 0.25) == 1.0 and host_test(2, 8, 0.25) == 1.0  # k == p * n
    # n = 2, p = 0.5: weights 1/4, 1/2, 1/4.  k = 0: itself and, on the far side, 2 (equal, within 1 + 1e-7)
    assert host_test(0, 2, 0.5) == 0.5 and host_test(2, 2, 0.5) == 0.5
    assert host_test(0, 1, 0.5) == 1.0 and host_test(1, 1, 0.5) == 1.0
    # n = 3, p = 0.25: 27/64, 27/64, 9/64, 1/64.  k = 2 > 0.75: 2 and 3 by index, nothing at or below floor(0.75) = 0 is as small
    assert close(host_test(2, 3, 0.25), 10 / 64) and close(host_test(3, 3, 0.25), 1 / 64)
    assert host_test(0, 3, 0.25) == 1.0                                 # k = 0 < 0.75: 0 by index, and 1, 2, 3 are no larger
    # n = 4, p = 0.5: 1, 4, 6, 4, 1 sixteenths
    assert all(close(host_test(k, 4, 0.5), want) for k, want in enumerate([2 / 16, 10 / 16, 1.0, 10 / 16, 2 / 16])) and host_test(2, 4, 0.5) == 1.0
    # deep tails stay finite where they can and reach zero through the subnormals where they cannot
    # 603 ratios at the most between the anchor and a term, five roundings in each (two of them in r): 603 * 5 * 2 ** -53 = 3.4e-13
    exact = exact_test(568, 603, 0.2748)
    assert 2.2e-267 < exact < 2.3e-267 and abs(Fraction(host_test(568, 603, 0.2748)) - exact) <= Fraction(3.4e-13) * exact
    assert host_test(0, 4000, 0.5) == 0.0 and host_test(900, 2000, 0.02) < 1e-300
    assert close(host_test(0, 1000, 0.5), 2 * 0.5 ** 1000, rel=1e-12) and 2 * 0.5 ** 1000 < 1e-300


def test_the_three_error_codes_of_the_test_rule():
    from clairs_to_amd._lib import CtoError
    from clairs_to_amd.tag_germline_variant import binom_two_sided
    with pytest.raises(CtoError, match=r"item 1: n must be an integer not less than 1"):
        binom_two_sided([1, 0], [5, 0], [0.5, 0.5], "host")
    with pytest.raises(CtoError, match=r"item 0: k \(6\) must not be greater than n \(5\)\."):
        binom_two_sided([6], [5], [0.5], "host")
    with pytest.raises(CtoError, match=r"k must be an integer not less than 0"):
        binom_two_sided([-1], [5], [0.5], "host")
    for p in (-0.1, 1.5, NAN):
        with pytest.raises(CtoError, match=r"item 2: p \(.*\) must be in range \[0,1\]"):
            binom_two_sided([1, 1, 1], [5, 5, 5], [0.5, 0.5, p], "host")
    with pytest.raises(CtoError, match="where"):
        from clairs_to_amd._lib import check, lib
        check(lib.cto_binom_two_sided(None, None, None, 0, 2, None))
    assert binom_two_sided([], [], [], "host").shape == (0,)
    with pytest.raises(ValueError):
        binom_two_sided([1], [5], [0.5], "elsewhere")
    # the same through the call that tags: only a call with a segment is tested
    with pytest.raises(CtoError, match=r"item 1: k \(60\) must not be greater than n \(40\)"):
        host_calls([0, 0], [200, 200], [40, 40], [0.3, 1.5])
    with pytest.raises(CtoError, match=r"item 0: n must be"):
        host_calls([0], [200], [0], [0.3])
    with pytest.raises(CtoError, match=r"item 0: p must be in range"):
        host_calls([0], [200], [40], [0.3], purity=-3.0)
    seg, _, pv = host_calls([0, 0], [950, 950], [0, 40], [0.3, 1.5])
    assert seg.tolist() == [-1, -1] and np.isnan(pv).all()


VCF_HEAD = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n"
CNA = "Sample\tChromosome\tStartPosition\tEndPosition\tnMajor\tnMinor\nT\tchr1\t100\t900\t1\t1\n"
PURITY = "Sample\tPurity\tPloidy\tGoodnessOfFit\nT\t0.4\t2.0\t99.0\n"


def run_rows(tmp_path, rows, where="host"):
    from clairs_to_amd.__main__ import dispatch
    (tmp_path / "in.vcf").write_text(VCF_HEAD + "".join(rows))
    (tmp_path / "cna.txt").write_text(CNA)
    (tmp_path / "purity.txt").write_text(PURITY)
    out = str(tmp_path / "out.vcf")
    dispatch("tag_germline_variant", ["--input_vcf_fn", str(tmp_path / "in.vcf"), "--output_fn", out, "--tumor_purity_ploidy_output_file",
                                      str(tmp_path / "purity.txt"), "--tumor_cna_output_file", str(tmp_path / "cna.txt"), "--where", where])
    return output_text(out)


GOOD = "chr1\t500\t.\tA\tG\t20.0\tPASS\tH\tGT:GQ:DP:AF\t0/1:20:60:0.9800\n"


def test_where_the_reference_dies_we_name_the_row(tmp_path):
    assert run_rows(tmp_path, [GOOD]) == VCF_HEAD + GOOD.replace("PASS\tH", "LowQual\tH;Verdict_Germline")
    no_af = "chr1\t510\t.\tA\tG\t20.0\tPASS\tH\tGT:GQ:DP\t0/1:20:60\n"
    with pytest.raises(SystemExit, match=r"no AF or VAF field .*chr1\\t510"):
        run_rows(tmp_path, [GOOD, no_af])
    outside = no_af.replace("510", "1510")                              # no segment holds it: the reference never looks at its AF
    assert run_rows(tmp_path, [GOOD, outside]).endswith(outside)
    with pytest.raises(SystemExit, match=r"no integer depth .*chr1\\t520"):
        run_rows(tmp_path, [GOOD, "chr1\t520\t.\tA\tG\t20.0\tPASS\tH\tGT:GQ:DP:AF\t0/1:20:6.5:0.3000\n"])
    with pytest.raises(SystemExit, match=r"no integer depth .*chr1\\t9520"):                                 # with or without a segment
        run_rows(tmp_path, ["chr1\t9520\t.\tA\tG\t20.0\tPASS\tH\tGT:GQ\t0/1:20\n"])
    with pytest.raises(SystemExit, match=r"k \(90\) must not be greater than n \(60\)\. .*chr1\\t530"):
        run_rows(tmp_path, [GOOD, "chr1\t530\t.\tA\tG\t20.0\tPASS\tH\tGT:GQ:DP:AF\t0/1:20:60:1.5000\n"])
    not_pass = "chr1\t540\t.\tA\tG\t20.0\tLowQual\tH\tGT:GQ:DP\t0/1:20:x  \n"                              # not PASS: nothing of it is read
    assert run_rows(tmp_path, [not_pass, GOOD]).startswith(VCF_HEAD + not_pass)


def test_the_depth_is_the_third_field_and_vaf_stands_in_for_af(tmp_path):
    row = "chr1\t500\t.\tA\tG\t20.0\tPASS\t.\tGT:VAF:XX:DP\t0/1:0.9800:60:7 \n"
    assert run_rows(tmp_path, [row]) == VCF_HEAD + "chr1\t500\t.\tA\tG\t20.0\tLowQual\t.;Verdict_Germline\tGT:VAF:XX:DP\t0/1:0.9800:60:7\n"
    star = "chr1\t505\t.\tA\tG,*\t20.0\tPASS\t.\tGT:GQ:DP:AF\t0/1:9:60:0.9800\n"                          # the reader drops it, with a word
    assert run_rows(tmp_path, [star, GOOD]) == VCF_HEAD + GOOD.replace("PASS\tH", "LowQual\tH;Verdict_Germline")


class Recorder:
    def __init__(self, monkeypatch, fail=None):
        import importlib
        self.calls = []
        for name in ("allele_counter", "get_logr_and_baf", "correct_logr", "predict_germline_genotypes", "aspcf", "run_ascat", "tag_germline_variant"):
            mod = importlib.import_module("clairs_to_amd." + name)

            def main(argv=None, name=name):
                self.calls.append((name, list(argv)))
                if fail is not None and name == fail[0]:
                    raise fail[1]
                return 0
            monkeypatch.setattr(mod, "main", main)


def driver_argv(golden, tmp_path, extra=()):
    o = golden["commands"]["options"]
    (tmp_path / "contigs.txt").write_text(golden["commands"]["contig_file"])
    argv = []
    for k in ("python", "verdict", "parallel", "threads", "allele_counter", "tumor_bam_fn", "cna_resource_dir", "output_dir", "tumor_sample_name", "normal_sample_name",
              "contig_fn", "input_vcf_fn", "output_fn", "platform"):
        argv += ["--" + k, str(o[k])]
    return argv + list(extra)


def test_the_driver_hands_the_steps_the_reference_s_arguments(golden, tmp_path, monkeypatch):
    from clairs_to_amd.__main__ import dispatch
    monkeypatch.chdir(tmp_path)
    rec = Recorder(monkeypatch)
    dispatch("cna_germline_tagging", driver_argv(golden, tmp_path))
    strings = golden["commands"]["strings"]
    assert [c[0] for c in rec.calls] == ["allele_counter", "get_logr_and_baf", "correct_logr", "predict_germline_genotypes", "aspcf", "run_ascat", "tag_germline_variant"]
    for (name, argv), command in list(zip(rec.calls, strings))[1:]:
        words = shlex.split(command)
        assert words[1].endswith("/" + name + ".py") and argv == words[2:], name
    # step 1: alleleCounter's five options, and the three prefixes in place of GNU parallel's {1}
    words = shlex.split(strings[0])
    counter = words[words.index("/opt/ac/bin/alleleCounter") + 1:words.index(":::")]
    assert counter[counter.index("-m"):] == ["-m", "20", "-q", "20", "-f", "0", "-F", "2316", "--dense-snps"]
    assert rec.calls[0][1] == ["-b", "tumor.bam", "--contig_fn", "contigs.txt", "--loci_prefix", counter[3].split("{1}")[0], "--output_prefix",
                               counter[5].split("{1}")[0]] + counter[counter.index("-m"):]
    assert counter[:2] == ["-b", "tumor.bam"] and counter[3].endswith("{1}.txt") and counter[5].endswith("{1}.txt")
    assert words[words.index(":::") + 1:] == ["chr1", "chr2", "chrX", "chr21"]
    assert os.path.isdir("out")                                         # made when it is not there
    from clairs_to_amd import cna_germline_tagging
    import argparse
    assert cna_germline_tagging.commands(argparse.Namespace(**golden["commands"]["options"])) == strings


def test_with_is_indel_only_the_tagging_runs(golden, tmp_path, monkeypatch):
    from clairs_to_amd.__main__ import dispatch
    monkeypatch.chdir(tmp_path)
    rec = Recorder(monkeypatch)
    dispatch("cna_germline_tagging", driver_argv(golden, tmp_path, ["--is_indel"]))
    assert rec.calls == [("tag_germline_variant", shlex.split(golden["commands"]["strings"][6])[2:])]


@pytest.mark.parametrize("failure", [RuntimeError("no such table"), SystemExit("correct_logr: bad table"), SystemExit(3)])
def test_a_step_that_fails_gives_the_reference_s_line_and_exit_1(golden, tmp_path, monkeypatch, capsys, failure):
    from clairs_to_amd.__main__ import dispatch
    monkeypatch.chdir(tmp_path)
    rec = Recorder(monkeypatch, fail=("correct_logr", failure))
    with pytest.raises(SystemExit) as e:
        dispatch("cna_germline_tagging", driver_argv(golden, tmp_path))
    assert e.value.code == 1 and [c[0] for c in rec.calls] == ["allele_counter", "get_logr_and_baf", "correct_logr"]
    err = capsys.readouterr().err
    assert err.endswith("ERROR in STEP 3, THE FOLLOWING COMMAND FAILED: {}\n".format((golden["commands"]["strings"][2],)))
    rec = Recorder(monkeypatch, fail=("tag_germline_variant", failure))
    with pytest.raises(SystemExit) as e:
        dispatch("cna_germline_tagging", driver_argv(golden, tmp_path, ["--is_indel"]))
    assert e.value.code == 1
    assert capsys.readouterr().err.endswith("ERROR in STEP 1, THE FOLLOWING COMMAND FAILED: {}\n".format(golden["commands"]["strings"][6]))
