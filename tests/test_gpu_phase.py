"""cto_phase_reads, device path (csrc/phase.hip) against the host path: the observations, the link table, the phases and the reads' tags,
array for array - integers only, so every comparison is exact.  What the host path itself is held to: tests/test_phase_reads.py."""
import pytest

import phaseutil as pu
from test_phase_reads import sites_args

pytestmark = pytest.mark.gpu

CHUNK_BYTES = "40000"                          # CTO_PHASE_CHUNK_BYTES that cuts a simulated contig into several chunks


def both(bam, ctg, sites, **kw):
    from clairs_to_amd.phase_tumor import phase_reads
    st_h, st_d = {}, {}
    host = phase_reads(bam, ctg, *sites_args(sites), where="host", stats=st_h, **kw)
    dev = phase_reads(bam, ctg, *sites_args(sites), where="device", stats=st_d, **kw)
    return host, dev, st_h, st_d


@pytest.fixture(scope="module")
def bams(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_phase")
    out = {}
    for level in (0, 6):
        reads, info = pu.write_hand_bam(d / ("hand_l%d.bam" % level), level=level)
        out["hand", level] = dict(bam=str(d / ("hand_l%d.bam" % level)), ctg=pu.HAND_CTG, sites=pu.HAND_SITES, reads=reads, info=info)
    for seed in pu.SIM_SEEDS:
        case = pu.sim_case(seed)
        for level in (0, 6):
            bam = d / ("sim%d_l%d.bam" % (seed, level))
            info = pu.write_sim_bam(bam, case, level=level)
            out[seed, level] = dict(bam=str(bam), ctg=pu.SIM_CTG, sites=case["sites"], reads=case["reads"], info=info)
    return out


@pytest.mark.parametrize("level", [0, 6])
@pytest.mark.parametrize("which", ["hand"] + list(pu.SIM_SEEDS))
def test_device_equals_host(bams, which, level):
    b = bams[which, level]
    host, dev, st_h, st_d = both(b["bam"], b["ctg"], b["sites"])
    pu.assert_same_arrays(host, dev)
    assert st_d["fallback_chunks"] == 0 and st_d["n_blocks"] > 0 and st_d["inflated_bytes"] > 0
    assert st_d["n_phase_blocks"] == st_h["n_phase_blocks"] >= 1
    assert len(dev["voff"]) >= (17 if which == "hand" else 350) and len(dev["obs"]) > 30
    if which == "hand":                                   # and the values written out by hand
        got = pu.shaped(dev, 8)
        assert got["obs"] == [o for _, o in pu.HAND_OBS] and got["link"] == pu.HAND_LINK
        assert got["phase"] == pu.HAND_PHASE and got["ps"] == pu.HAND_PS
        voff = pu.voffs_of(b["info"])
        name_of = {voff[i]: r["name"] for i, r in enumerate(b["reads"])}
        assert {name_of[v]: t for v, t in zip(got["voff"], got["tags"])} == pu.HAND_TAGS


@pytest.mark.parametrize("seed", [7, 23])
def test_chunk_boundaries(bams, seed, monkeypatch):
    b = bams[seed, 6]
    host, one, _, st_one = both(b["bam"], b["ctg"], b["sites"])
    assert st_one["n_chunks"] == 1 and st_one["n_merged_reads"] == 0
    monkeypatch.setenv("CTO_PHASE_CHUNK_BYTES", CHUNK_BYTES)
    host_cut, cut, st_h, st_d = both(b["bam"], b["ctg"], b["sites"])
    assert st_d["n_chunks"] >= 4 and st_d["n_merged_reads"] > 50 and st_d["fallback_chunks"] == 0
    assert st_d["n_reads_entered"] > len(cut["voff"]) == len(one["voff"])
    assert st_h["n_chunks"] == st_d["n_chunks"] and st_h["n_merged_reads"] == st_d["n_merged_reads"]
    pu.assert_same_arrays(one, cut)
    pu.assert_same_arrays(host, cut)
    pu.assert_same_arrays(host, host_cut)


def test_every_site_a_chunk_on_the_hand_built_bam(bams, monkeypatch):
    b = bams["hand", 6]
    host, _, _, _ = both(b["bam"], b["ctg"], b["sites"])
    monkeypatch.setenv("CTO_PHASE_CHUNK_BYTES", "1")
    _, cut, _, st_d = both(b["bam"], b["ctg"], b["sites"])
    assert st_d["n_chunks"] >= 2 and st_d["n_merged_reads"] >= 1
    pu.assert_same_arrays(host, cut)


@pytest.mark.parametrize("level", [0, 6])
def test_link_span(bams, level):
    b = bams["hand", level]
    h1, d1, _, s1 = both(b["bam"], b["ctg"], b["sites"], link_span=1)
    h8, d8, _, s8 = both(b["bam"], b["ctg"], b["sites"], link_span=8)
    pu.assert_same_arrays(h1, d1)
    pu.assert_same_arrays(h8, d8)
    assert list(d8["ps"][:6]) == [100, 100, 100, 0, 100, 100] and s8["n_phase_blocks"] == 2          # K = 8 bridges the unphased site
    assert list(d1["ps"][:6]) == [100, 100, 100, 0, 500, 500] and s1["n_phase_blocks"] == 3          # K = 1 breaks the block there


def test_phase_tumor_device_writes_the_hosts_files(tmp_path):
    from test_phase_tumor_cli import input_vcf, run_cli
    case = pu.sim_case(11)
    pu.write_sim_bam(tmp_path / "t.bam", case)
    (tmp_path / "vcf").mkdir()
    (tmp_path / "vcf" / (pu.SIM_CTG + ".vcf")).write_text(input_vcf(case))
    hv, hb = run_cli(tmp_path, "host", "host")
    dv, db = run_cli(tmp_path, "device", "device")
    for a, b in ((hv, dv), (hb, db), (hb + ".bai", db + ".bai")):
        assert open(a, "rb").read() == open(b, "rb").read(), (a, b)
    assert len(open(db, "rb").read()) > 100000
