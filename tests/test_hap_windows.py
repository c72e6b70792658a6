"""Haplotype windows from the BAM, host path (cto_hap_windows, where = host: csrc/bam.cpp hap_windows_host; the job object and its
two halves: csrc/hapfilter.cpp).  The reference's own output VCF (tests/golden/hapfilter*.json.gz) is reached from BAM files written
from the fixtures' simulation, with no text anywhere; the job itself is compared with the one the nine-column text parses to, through
cto_hap_job_view.  Integers and bytes only: every comparison is exact.  No GPU needed."""
import numpy as np
import pytest

import bamutil
import haputil
from conftest import load_json_gz

import hapsim                      # tests/golden, on the path through haputil
import gen_hapfilter_wide as gw


def _jobs():
    from clairs_to_amd.haplotype_filtering import HapJob
    return HapJob


@pytest.fixture(scope="module")
def seed7(tmp_path_factory):
    d = tmp_path_factory.mktemp("hap7")
    sim = hapsim.simulate(seed=7)
    bam = d / "t.bam"
    bamutil.write_bam(str(bam), [("chr1", len(sim["ref"]))], haputil.reads_of(sim), block_payload=30000)
    return dict(dir=d, sim=sim, bam=bam, golden=load_json_gz("hapfilter.json.gz"))


@pytest.mark.parametrize("mode", ["snv", "indel"])
def test_host_job_equals_the_job_of_the_text(seed7, mode):
    """column for column, record for record: key string, base, indel bytes, BQ, MQ, hp, hp_single, start / end lists.  One field is
    left out for `*` / `#` records: hapsim gives a deleted base its own position's quality, csrc/bam.cpp's rule the quality of the
    query base behind the deletion - and no rule of the evaluation reads the BQ of a placeholder."""
    HapJob = _jobs()
    text = seed7["golden"]["modes"][mode]["mpileup"]
    pos = haputil.rows_positions(text)
    assert text == hapsim.pileup_rows(seed7["sim"], pos), "the simulator changed: regenerate tests/golden/hapfilter.json.gz"
    lo, hi = pos[0], pos[-1]
    with HapJob.from_text(text, lo, hi) as jt, HapJob.from_bam(seed7["bam"], "chr1", lo, hi, haputil.merged_intervals(pos), reverse_del=True,
                                                                where="host") as jb:
        want, got = haputil.job_columns(jt.view(), False), haputil.job_columns(jb.view(), False)
        assert jb.view()["lo"] == lo and jb.view()["hi"] == hi
    assert len(want) == len(pos)
    assert got == want, haputil.first_difference(got, want)
    assert mode != "snv" or any(len(r[2]) > 280 for c in want for r in c[1]), "the 300-base insertion of the variant-cluster case must be in there"


@pytest.mark.parametrize("mode", ["snv", "indel"])
def test_cli_from_the_bam_writes_the_reference_vcf_whatever_the_job_cut(seed7, mode):
    from clairs_to_amd.haplotype_filtering import haplotype_filter
    g, d = seed7["golden"], seed7["dir"]
    haputil.write_inputs(d, "chr1", g["ref"], g["germline_vcf"], g["modes"][mode]["pileup_vcf"])
    want = g["modes"][mode]["out_vcf"]
    for sites in (1, 3, 200):
        for bed in (True, False):
            name = "out_%s_%d_%d.vcf" % (mode, sites, bed)
            res = haplotype_filter(haputil.stage_args(d, "chr1", seed7["bam"], mode, name, "host", haplotype_chunk_max_sites=sites,
                                                      haplotype_chunk_mpileup_bed=bed))
            assert (d / name).read_text() == want, (sites, bed)
            assert len(res) >= (20 if mode == "snv" else 5)


def test_cli_phased_prefix_and_text_precedence(seed7, tmp_path):
    """<prefix><ctg>.bam resolves as in the samtools path; --mpileup_fn still wins over --pileup_source bam"""
    import shutil
    from clairs_to_amd.haplotype_filtering import haplotype_filter
    g = seed7["golden"]
    haputil.write_inputs(tmp_path, "chr1", g["ref"], g["germline_vcf"], g["modes"]["snv"]["pileup_vcf"])
    shutil.copy(str(seed7["bam"]), str(tmp_path / "phased_chr1.bam"))
    shutil.copy(str(seed7["bam"]) + ".bai", str(tmp_path / "phased_chr1.bam.bai"))
    haplotype_filter(haputil.stage_args(tmp_path, "chr1", tmp_path / "phased_", "snv", "a.vcf", "host"))
    assert (tmp_path / "a.vcf").read_text() == g["modes"]["snv"]["out_vcf"]
    (tmp_path / "mp.txt").write_text(g["modes"]["snv"]["mpileup"])
    haplotype_filter(haputil.stage_args(tmp_path, "chr1", "no_such.bam", "snv", "b.vcf", "host", mpileup_fn=str(tmp_path / "mp.txt")))
    assert (tmp_path / "b.vcf").read_text() == g["modes"]["snv"]["out_vcf"]


def test_cli_options_parse():
    from clairs_to_amd.haplotype_filtering import build_parser
    a = build_parser().parse_args([])
    assert a.pileup_source == "samtools" and a.where is None
    a = build_parser().parse_args(["--pileup_source", "bam", "--where", "host"])
    assert a.pileup_source == "bam" and a.where == "host"


def test_wide_fixture_from_bams(tmp_path):
    """every contig of tests/golden/hapfilter_wide.json.gz, both passes, from a BAM: the reference's own files; one job without the
    BED for the SNV pass, jobs of three calls with it for the indel pass"""
    from clairs_to_amd.haplotype_filtering import haplotype_filter
    g = load_json_gz("hapfilter_wide.json.gz")
    assert len(g["contigs"]) >= 16
    for rec in g["contigs"]:
        ctg = rec["name"]
        sim = hapsim.simulate(seed=rec["seed"])
        inputs = haputil.wide_inputs(sim, ctg)
        d = tmp_path / ("c%d" % rec["seed"])
        d.mkdir()
        bam = d / "t.bam"
        bamutil.write_bam(str(bam), [(ctg, len(sim["ref"]))], haputil.reads_of(sim), block_payload=60000, level=1)
        for mode in ("snv", "indel"):
            haputil.write_inputs(d, ctg, sim["ref"], gw.germline_vcf(sim, ctg), inputs[mode])
            over = dict(haplotype_chunk_max_sites=3) if mode == "indel" else dict(haplotype_chunk_mpileup_bed=False)
            haplotype_filter(haputil.stage_args(d, ctg, bam, mode, "out_%s.vcf" % mode, "host", **over))
            assert (d / ("out_%s.vcf" % mode)).read_text() == rec[mode]["out_vcf"], (ctg, mode)


# ------------------------------------------------------------------------------------------ the BAM written out by hand
@pytest.fixture(scope="module")
def hand(tmp_path_factory):
    d = tmp_path_factory.mktemp("hand")
    bam = d / "hand.bam"
    info = bamutil.write_bam(str(bam), [(haputil.HAND_CTG, haputil.HAND_LEN)], haputil.hand_reads(), block_payload=97)
    sizes = info["block_sizes"]
    assert any(a // 97 != (b - 1) // 97 for a, b in info["record_spans"]), "records must straddle BGZF blocks"
    assert len(sizes) > 20
    return bam


def _hand_pair(bam, covers_text, lo, hi, wanted, **kw):
    HapJob = _jobs()
    with HapJob.from_text(covers_text, lo, hi) as jt, HapJob.from_bam(bam, haputil.HAND_CTG, lo, hi, haputil.merged_intervals(wanted), where="host",
                                                                      **kw) as jb:
        return haputil.job_columns(jb.view()), haputil.job_columns(jt.view()), jb.stats


@pytest.mark.parametrize("reverse_del", [0, 1])
@pytest.mark.parametrize("min_bq", [0, 10])
def test_hand_built_bam_against_rows_written_by_hand(hand, reverse_del, min_bq):
    text = haputil.hand_rows(haputil.hand_covers(reverse_del), min_bq)
    got, want, _ = _hand_pair(hand, text, 1, haputil.HAND_LEN, haputil.HAND_WANTED, min_mq=20, min_bq=min_bq, max_depth=0, reverse_del=reverse_del)
    assert got == want, haputil.first_difference(got, want)
    cols = dict((c[0], c) for c in got)
    # what the rows say, spelled out where it is easy to get wrong
    assert (11 in cols) == (min_bq == 0) and (30 in cols) == (min_bq == 0)           # head and tail base below min_bq: nothing prints
    e_del = [r for r in cols[19][1] if r[1] in "*#"][0]
    assert e_del[1] == ("#" if reverse_del else "*")
    # behind n's skip the bases pair with the names one place ahead: e's deletion carries n's name, on the strand its character says
    assert e_del[0] == ("n_1" if reverse_del else "n_0")
    assert [r[2] for r in cols[18][1] if r[2]] == [b"-nn"] and cols[111][1][0][2] == b"+C" and cols[327][1][0][2] == b"-n"
    assert cols[1][2] == [-1] and cols[5][2] == [0] and cols[133][2] == [0] and cols[329][2] == [0]
    if min_bq == 0:
        b12 = cols[12][1][1]
        assert b12[:2] == ("b_1", "N") and b12[3] == 0 and (b12[5], b12[6]) == ("1", 0)      # `=` reads as N, no QUAL is 0, HP 12 is two characters
        assert [r[0] for r in cols[16][1]] == ["a_0", "b_1", "d_0", "d_0", "n_0", "e_1"]    # the same qname twice: one id


def test_hand_built_bam_depth_cap_clipping_and_empty_job(hand):
    covers = haputil.hand_covers(1)
    # max_depth = 4 under six covers: the fifth and sixth read find four reads open at their start
    text = haputil.hand_rows({360: covers[360]}, keep=("m1", "m2", "m3", "m4"))
    got, want, _ = _hand_pair(hand, text, 340, 400, [360], max_depth=4, reverse_del=1)
    assert got == want and len(got[0][1]) == 4
    got, want, _ = _hand_pair(hand, haputil.hand_rows({360: covers[360]}), 340, 400, [360], max_depth=6, reverse_del=1)
    assert got == want and len(got[0][1]) == 6
    # intervals reach over both ends of the region: clipped at position 1 and at region_hi
    HapJob = _jobs()
    with HapJob.from_bam(hand, haputil.HAND_CTG, 1, 3, [[0, 50]], where="host", max_depth=0) as j:
        assert [c[0] for c in haputil.job_columns(j.view())] == [1, 2, 3]
    # a job no read covers
    with HapJob.from_bam(hand, haputil.HAND_CTG, 380, 390, None, where="host") as j:
        v = j.view()
        assert len(v["col_pos"]) == 0 and len(v["recs"]) == 0 and j.stats["n_recs"] == 0
        assert j.evaluate("A" * 11, 380, [], 100, 2, False) == []
    # no intervals = every position of the region
    with HapJob.from_bam(hand, haputil.HAND_CTG, 1, haputil.HAND_LEN, None, where="host", max_depth=0, reverse_del=1) as j:
        whole = dict((c[0], c) for c in haputil.job_columns(j.view()))
    with HapJob.from_text(haputil.hand_rows(covers), 1, haputil.HAND_LEN) as jt:
        for c in haputil.job_columns(jt.view()):
            assert whole[c[0]] == c


def test_bad_arguments_are_errors(hand):
    from clairs_to_amd._lib import CtoError
    HapJob = _jobs()
    with pytest.raises(CtoError):
        HapJob.from_bam(hand, haputil.HAND_CTG, 10, 5, None, where="host")
    with pytest.raises(CtoError):
        HapJob.from_bam(hand, haputil.HAND_CTG, 1, 100, [[50, 60], [10, 20]], where="host")
    with pytest.raises(CtoError):
        HapJob.from_bam(hand, "nope", 1, 100, None, where="host")
    with pytest.raises(ValueError):
        HapJob.from_bam(hand, haputil.HAND_CTG, 1, 100, None, where="nowhere")


@pytest.mark.parametrize("mode", ["snv", "indel"])
def test_one_call_equals_its_two_halves(mode):
    """cto_haplotype_filter on the fixture text == cto_hap_job_from_text + cto_hap_evaluate, flag for flag"""
    from clairs_to_amd.haplotype_filtering import HapJob, evaluate_job, read_vcf
    g = load_json_gz("hapfilter.json.gz")
    m = g["modes"][mode]
    calls = []
    for row in m["pileup_vcf"].split("\n"):
        c = row.split("\t")
        if row and row[0] != "#" and c[6] == "PASS" and ((len(c[3]) == 1 and len(c[4]) == 1) == (mode == "snv")):
            calls.append((int(c[1]), c[3], c[4], 0.2, "", ""))
    assert len(calls) >= 5
    lo, hi = max(1, calls[0][0] - 100), calls[-1][0] + 100
    ref = g["ref"][lo - 1:hi + 1]
    one = evaluate_job(m["mpileup"], ref, lo, calls, 100, 2, False)
    with HapJob.from_text(m["mpileup"], lo, hi) as j:
        two = j.evaluate(ref, lo, calls, 100, 2, False)
    assert one == two and any(not r["pass_hap"] for r in one) and any(r["pass_hap"] for r in one)
