"""Haplotype windows from the BAM, device path (csrc/hapwindows.hip): the job cto_hap_windows builds on the device is the job its host
rules build (tests/test_hap_windows.py holds those against the text and the reference), array for array through cto_hap_job_view,
and the stage writes the reference's own VCF from it.  Integers and bytes only: every comparison is exact."""
import shutil

import numpy as np
import pytest

import bamutil
import haputil
from conftest import load_json_gz

import hapsim
import gen_hapfilter_wide as gw

pytestmark = pytest.mark.gpu


def _job(bam, ctg, lo, hi, iv, where, **kw):
    from clairs_to_amd.haplotype_filtering import HapJob
    with HapJob.from_bam(bam, ctg, lo, hi, iv, where=where, **kw) as j:
        return j.view(), j.stats


def _same_view(a, b):
    assert a["keys"] == b["keys"] and a["indels"] == b["indels"] and (a["lo"], a["hi"]) == (b["lo"], b["hi"])
    for k in ("col_pos", "col_off", "rse_off", "rse"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert a["recs"].tobytes() == b["recs"].tobytes()


@pytest.fixture(scope="module")
def seed7(tmp_path_factory):
    """the fixture's contig at deflate level 6 and, stored, at level 0; behind it a second contig whose blocks the span of chr1 holds
    and chr1's reads do not"""
    d = tmp_path_factory.mktemp("hap7gpu")
    sim = hapsim.simulate(seed=7)
    reads = haputil.reads_of(sim)
    tail = [dict(name="t%d" % i, flag=0, ref=1, pos=10 * i, mapq=60, cigar=[("M", 3000)], seq="ACGT" * 750, qual=[30] * 3000, aux=b"") for i in range(30)]
    refs = [("chr1", len(sim["ref"])), ("chr2", 5000)]
    info = bamutil.write_bam(str(d / "l6.bam"), refs, reads + tail, block_payload=30000, level=6)
    bamutil.write_bam(str(d / "l0.bam"), refs, reads + tail, block_payload=30000, level=0)
    return dict(dir=d, sim=sim, l6=d / "l6.bam", l0=d / "l0.bam", info=info, n_chr1=len(reads), golden=load_json_gz("hapfilter.json.gz"))


@pytest.mark.parametrize("level", ["l0", "l6"])
@pytest.mark.parametrize("mode", ["snv", "indel"])
def test_device_job_equals_host_job_on_the_fixture(seed7, mode, level):
    pos = haputil.rows_positions(seed7["golden"]["modes"][mode]["mpileup"])
    iv = haputil.merged_intervals(pos)
    dev, st = _job(seed7[level], "chr1", pos[0], pos[-1], iv, "device", reverse_del=True)
    host, _ = _job(seed7[level], "chr1", pos[0], pos[-1], iv, "host", reverse_del=True)
    _same_view(dev, host)
    assert st["n_chunks"] == 1 and st["fallback_chunks"] == 0 and st["cap_chunks"] == 0 and st["host_columns"] == 0
    assert st["n_recs"] == len(host["recs"]) > 10000 and st["n_blocks"] > 5


def test_device_twice_gives_identical_bytes_and_chunks_change_nothing(seed7, monkeypatch):
    a, _ = _job(seed7["l6"], "chr1", 1, 9000, None, "device", reverse_del=True, max_depth=0)
    b, _ = _job(seed7["l6"], "chr1", 1, 9000, None, "device", reverse_del=True, max_depth=0)
    _same_view(a, b)
    monkeypatch.setenv("CTO_HAP_CHUNK_BYTES", "200000")
    c, st = _job(seed7["l6"], "chr1", 1, 9000, None, "device", reverse_del=True, max_depth=0)
    assert st["n_chunks"] >= 2 and st["fallback_chunks"] == 0 and st["cap_chunks"] == 0
    _same_view(a, c)
    # under a cap the chunks behind the first are the host's, and say so
    e, st = _job(seed7["l6"], "chr1", 1, 9000, None, "device", reverse_del=True, max_depth=8000)
    assert st["cap_chunks"] == st["n_chunks"] - 1 >= 1
    _same_view(a, e)


@pytest.mark.parametrize("reverse_del", [0, 1])
@pytest.mark.parametrize("min_bq", [0, 10])
def test_device_job_equals_host_job_on_the_hand_built_bam(tmp_path, reverse_del, min_bq):
    bam = tmp_path / "hand.bam"
    bamutil.write_bam(str(bam), [(haputil.HAND_CTG, haputil.HAND_LEN)], haputil.hand_reads(), block_payload=97)
    iv = haputil.merged_intervals(haputil.HAND_WANTED)
    kw = dict(min_mq=20, min_bq=min_bq, max_depth=0, reverse_del=reverse_del)
    dev, st = _job(bam, haputil.HAND_CTG, 1, haputil.HAND_LEN, iv, "device", **kw)
    host, _ = _job(bam, haputil.HAND_CTG, 1, haputil.HAND_LEN, iv, "host", **kw)
    _same_view(dev, host)
    assert st["host_columns"] == 3 and st["fallback_chunks"] == 0          # columns 17, 18, 19 lie under read n's skip
    from clairs_to_amd.haplotype_filtering import HapJob
    with HapJob.from_text(haputil.hand_rows(haputil.hand_covers(reverse_del), min_bq), 1, haputil.HAND_LEN) as jt:
        assert haputil.job_columns(dev) == haputil.job_columns(jt.view())
    # every position, so that the skip's columns sit between device columns on both sides
    dev, st = _job(bam, haputil.HAND_CTG, 1, haputil.HAND_LEN, None, "device", **kw)
    host, _ = _job(bam, haputil.HAND_CTG, 1, haputil.HAND_LEN, None, "host", **kw)
    _same_view(dev, host)
    assert st["host_columns"] == 3


def test_depth_cap_on_the_device(tmp_path):
    """max_depth = 4 under six covers: the cap comes into play, the chunk is the host's and is counted; at 6 it stays on the device"""
    bam = tmp_path / "hand.bam"
    bamutil.write_bam(str(bam), [(haputil.HAND_CTG, haputil.HAND_LEN)], haputil.hand_reads(), block_payload=97)
    dev, st = _job(bam, haputil.HAND_CTG, 340, 400, [[359, 360]], "device", max_depth=4)
    host, _ = _job(bam, haputil.HAND_CTG, 340, 400, [[359, 360]], "host", max_depth=4)
    _same_view(dev, host)
    assert st["cap_chunks"] == 1 and len(dev["recs"]) == 4
    dev, st = _job(bam, haputil.HAND_CTG, 340, 400, [[359, 360]], "device", max_depth=7)
    assert st["cap_chunks"] == 0 and len(dev["recs"]) == 6
    dev, st = _job(bam, haputil.HAND_CTG, 380, 390, None, "device")
    assert len(dev["col_pos"]) == 0 and len(dev["recs"]) == 0


@pytest.mark.parametrize("mode", ["snv", "indel"])
def test_cli_on_the_device_writes_the_reference_vcf(seed7, mode):
    from clairs_to_amd.haplotype_filtering import haplotype_filter
    g, d = seed7["golden"], seed7["dir"]
    haputil.write_inputs(d, "chr1", g["ref"], g["germline_vcf"], g["modes"][mode]["pileup_vcf"])
    for name, over in (("dev_a_%s.vcf" % mode, {}), ("dev_b_%s.vcf" % mode, dict(haplotype_chunk_max_sites=3, haplotype_chunk_mpileup_bed=False))):
        haplotype_filter(haputil.stage_args(d, "chr1", seed7["l6"], mode, name, "device", **over))
        assert (d / name).read_text() == g["modes"][mode]["out_vcf"], name


def test_cli_on_the_device_four_contigs_of_the_wide_fixture(tmp_path):
    from clairs_to_amd.haplotype_filtering import haplotype_filter
    g = load_json_gz("hapfilter_wide.json.gz")
    for k, rec in enumerate(g["contigs"][:4]):
        ctg = rec["name"]
        sim = hapsim.simulate(seed=rec["seed"])
        inputs = haputil.wide_inputs(sim, ctg)
        d = tmp_path / ("c%d" % rec["seed"])
        d.mkdir()
        bamutil.write_bam(str(d / "t.bam"), [(ctg, len(sim["ref"]))], haputil.reads_of(sim), block_payload=60000, level=(0, 6)[k & 1])
        for mode in ("snv", "indel"):
            haputil.write_inputs(d, ctg, sim["ref"], gw.germline_vcf(sim, ctg), inputs[mode])
            haplotype_filter(haputil.stage_args(d, ctg, d / "t.bam", mode, "out_%s.vcf" % mode, "device"))
            assert (d / ("out_%s.vcf" % mode)).read_text() == rec[mode]["out_vcf"], (ctg, mode)


def test_a_corrupted_crc_sends_the_chunk_to_the_host(seed7, tmp_path):
    """one flipped bit in the CRC-32 of a BGZF block that chr1's byte range holds and chr1's reads do not (it belongs to chr2): the device
    declines the chunk, the host path - which never opens that block - builds the job"""
    info = seed7["info"]
    end_chr1 = info["record_spans"][seed7["n_chr1"] - 1][1]
    k = next(i for i in range(len(info["block_sizes"])) if i * 30000 >= end_chr1)
    raw = bytearray(open(str(seed7["l6"]), "rb").read())
    raw[info["block_offsets"][k + 1] - 8] ^= 0x10
    bad = tmp_path / "bad.bam"
    bad.write_bytes(bytes(raw))
    shutil.copy(str(seed7["l6"]) + ".bai", str(bad) + ".bai")
    pos = haputil.rows_positions(seed7["golden"]["modes"]["snv"]["mpileup"])
    iv = haputil.merged_intervals(pos)
    dev, st = _job(bad, "chr1", pos[0], pos[-1], iv, "device", reverse_del=True)
    assert st["fallback_chunks"] == 1 and st["n_chunks"] == 1
    good, _ = _job(seed7["l6"], "chr1", pos[0], pos[-1], iv, "host", reverse_del=True)
    _same_view(dev, good)
