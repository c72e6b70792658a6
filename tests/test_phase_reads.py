"""cto_phase_reads, host path (csrc/bam.cpp): against the rules written out by hand and restated naively (tests/phaseutil.py) on a BAM
built by hand, and against simulated truth (tests/golden/hapsim.py).  PARITY UNPINNED against longphase and whatshap: the rules are the
definition (csrc/phase.hip).  No GPU."""
import pytest

import phaseutil as pu

from clairs_to_amd.phase_tumor import phase_reads


def sites_args(sites):
    return [s[0] for s in sites], [s[1] for s in sites], [s[2] for s in sites]


@pytest.fixture(scope="module")
def hand(tmp_path_factory):
    bam = tmp_path_factory.mktemp("phase_hand") / "hand.bam"
    reads, info = pu.write_hand_bam(bam)
    return dict(bam=str(bam), reads=reads, info=info)


def test_records_straddle_blocks(hand):
    info = hand["info"]
    assert max(info["block_sizes"]) == pu.HAND_BLOCK_PAYLOAD and len(info["block_sizes"]) > 50
    starts = {0}
    for s in info["block_sizes"]:
        starts.add(max(starts) + s)
    assert sum(1 for a, b in info["record_spans"] if any(a < x < b for x in starts)) >= len(hand["reads"])       # every record is cut


def test_hand_built_bam_against_the_rules_by_hand(hand):
    stats = {}
    got = pu.shaped(phase_reads(hand["bam"], pu.HAND_CTG, *sites_args(pu.HAND_SITES), where="host", stats=stats), 8)
    voff = pu.voffs_of(hand["info"])
    name_of = {voff[i]: r["name"] for i, r in enumerate(hand["reads"])}
    names = [name_of[v] for v in got["voff"]]
    assert names == [n for n, _ in pu.HAND_OBS]                          # the entered reads, in file order: not Q1, F1, O1
    assert got["obs"] == [o for _, o in pu.HAND_OBS]
    assert got["link"] == pu.HAND_LINK
    assert got["phase"] == pu.HAND_PHASE                                   # site 400 stays unphased
    assert got["ps"] == pu.HAND_PS                                         # two blocks, two PS values
    assert dict(zip(names, got["tags"])) == pu.HAND_TAGS
    assert stats["n_phase_blocks"] == 2 and stats["n_reads_entered"] >= 17 and stats["n_chunks"] >= 1


def test_hand_built_bam_against_the_restatement(hand):
    voff = pu.voffs_of(hand["info"])
    for K in (1, 2, 8):
        nv = pu.naive(hand["reads"], 0, pu.HAND_SITES, K=K)
        got = pu.shaped(phase_reads(hand["bam"], pu.HAND_CTG, *sites_args(pu.HAND_SITES), link_span=K, where="host"), K)
        assert got["voff"] == [voff[i] for i in nv["entered"]]
        for k in ("obs", "link", "phase", "ps", "tags"):
            assert got[k] == nv[k], (K, k)
    # the by-hand values are the restatement's too
    nv = pu.naive(hand["reads"], 0, pu.HAND_SITES)
    assert nv["obs"] == [o for _, o in pu.HAND_OBS] and nv["link"] == pu.HAND_LINK and nv["phase"] == pu.HAND_PHASE and nv["ps"] == pu.HAND_PS


def test_link_span_one_breaks_at_the_unphased_site(hand):
    k1 = phase_reads(hand["bam"], pu.HAND_CTG, *sites_args(pu.HAND_SITES), link_span=1, where="host")
    k8 = phase_reads(hand["bam"], pu.HAND_CTG, *sites_args(pu.HAND_SITES), link_span=8, where="host")
    assert list(k8["ps"][:6]) == [100, 100, 100, 0, 100, 100]             # K = 8 bridges site 400
    assert list(k1["ps"][:6]) == [100, 100, 100, 0, 500, 500]             # K = 1 cannot see past it
    assert k1["link"].shape == (8, 1, 2) and k8["link"].shape == (8, 8, 2)


def test_chunks_and_threads_change_nothing(hand, monkeypatch):
    one = phase_reads(hand["bam"], pu.HAND_CTG, *sites_args(pu.HAND_SITES), where="host", host_threads=1)
    monkeypatch.setenv("CTO_PHASE_CHUNK_BYTES", "1")                      # every site a chunk of its own
    stats = {}
    many = phase_reads(hand["bam"], pu.HAND_CTG, *sites_args(pu.HAND_SITES), where="host", host_threads=3, stats=stats)
    assert stats["n_chunks"] >= 2 and stats["n_merged_reads"] >= 1
    pu.assert_same_arrays(one, many)


def test_arguments_are_checked(hand):
    from clairs_to_amd._lib import CtoError
    pos, ref, alt = sites_args(pu.HAND_SITES)
    with pytest.raises(CtoError, match="strictly ascending"):
        phase_reads(hand["bam"], pu.HAND_CTG, [100, 100], "AA", "CC", where="host")
    with pytest.raises(CtoError, match="link_span"):
        phase_reads(hand["bam"], pu.HAND_CTG, pos, ref, alt, link_span=0, where="host")
    with pytest.raises(CtoError, match="not in the BAM header"):
        phase_reads(hand["bam"], "nope", pos, ref, alt, where="host")
    empty = phase_reads(hand["bam"], pu.HAND_CTG, [], [], [], where="host")
    assert len(empty["voff"]) == 0 and len(empty["phase"]) == 0 and list(empty["obs_off"]) == [0]


@pytest.mark.parametrize("seed", pu.SIM_SEEDS)
def test_quality_on_simulated_truth(seed, tmp_path):
    """The sites are the germline 0/1 SNPs plus the SNV calls, as a tumour-only VCF holds them.  Measured with the naive restatement
    when this was written: 0 switch errors; 20/20, 17/19, 17/19 germline SNPs phased; 382/390, 395/396, 377/382 eligible reads tagged;
    1/411, 0/419, 0/404 tagged reads wrong; 18, 21, 19 of the 26 calls left unphased."""
    case = pu.sim_case(seed)
    info = pu.write_sim_bam(tmp_path / "sim.bam", case)
    nv = pu.naive(case["reads"], 0, case["sites"])
    got = pu.shaped(phase_reads(str(tmp_path / "sim.bam"), pu.SIM_CTG, *sites_args(case["sites"]), where="host"), 8)
    voff = pu.voffs_of(info)
    assert got["voff"] == [voff[i] for i in nv["entered"]]
    for k in ("obs", "link", "phase", "ps", "tags"):
        assert got[k] == nv[k], k
    q = pu.quality(case, got, nv["entered"])
    print(seed, q)
    assert q["switch_errors"] == 0
    assert q["phased"] >= 0.85 * q["n_germline"]
    assert q["tagged_eligible"] >= 0.95 * q["eligible"] and q["eligible"] > 300
    assert q["wrong"] <= 0.01 * q["tagged"]
