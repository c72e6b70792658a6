"""cto_phase_reads, device path (csrc/phase.hip), past the first trip of its kernels' loops, on the BAM of tests/phaseshapes.py: more than
64 and 128 CIGAR operations per read (k_observe's carries and early exit), more than 64 sites under one operation, more than 64
observations per read and link spans up to the limit (k_link), more than 70 phase blocks with ties and threshold votes (k_assign), chunks
down to one site each (k_span), a damaged chunk, and the small ends.  Device against host array for array and against the naive
restatement - integers only, every comparison exact; no case may pass by going to the host.  The host path itself:
tests/test_phase_shapes.py."""
import numpy as np
import pytest

import phaseshapes as sh
import phaseutil as pu

pytestmark = pytest.mark.gpu

CASES = [(g, K) for g in sh.GROUPS + ("all",) for K in sh.LINK_SPANS]


def both(bam, sites, K=8, ctg=sh.CTG):
    from clairs_to_amd.phase_tumor import phase_reads
    args = [s[0] for s in sites], [s[1] for s in sites], [s[2] for s in sites]
    st_h, st_d = {}, {}
    host = phase_reads(bam, ctg, *args, link_span=K, where="host", stats=st_h)
    dev = phase_reads(bam, ctg, *args, link_span=K, where="device", stats=st_d)
    return host, dev, st_h, st_d


@pytest.fixture(scope="module")
def bams(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_phase_shapes")
    out = {}
    for level in (0, 6):
        bam = d / ("l%d.bam" % level)
        info = sh.write(bam, level=level)
        out[level] = dict(bam=str(bam), info=info)
    sh.write_damaged(out[0]["bam"], d / "bad.bam", out[0]["info"])
    out[0]["bad"] = str(d / "bad.bam")
    return out


@pytest.mark.parametrize("level", [0, 6])
@pytest.mark.parametrize("group,K", CASES)
def test_device_equals_host_and_the_restatement(bams, group, K, level):
    b = bams[level]
    host, dev, st_h, st_d = both(b["bam"], sh.case()["sites"][group], K)
    assert st_d["fallback_chunks"] == 0 and st_d["n_blocks"] > 0 and st_d["inflated_bytes"] > 0
    pu.assert_same_arrays(host, dev)
    assert st_d["n_phase_blocks"] == st_h["n_phase_blocks"] == sh.expected(group, K)["n_blocks"]
    assert st_d["n_chunks"] == st_h["n_chunks"] == 1 and st_d["n_merged_reads"] == 0
    got = sh.assert_matches_restatement(dev, group, K, b["info"])
    sh.assert_by_hand(got, group, K, b["info"])


@pytest.mark.parametrize("level", [0, 6])
@pytest.mark.parametrize("group,K,budget", sh.CUT_CASES)
def test_cut_into_chunks(bams, group, K, budget, level, monkeypatch):
    b = bams[level]
    monkeypatch.setenv("CTO_PHASE_CHUNK_BYTES", budget)
    host, dev, st_h, st_d = both(b["bam"], sh.case()["sites"][group], K)
    assert st_d["fallback_chunks"] == 0
    assert st_d["n_chunks"] == st_h["n_chunks"] and st_d["n_merged_reads"] == st_h["n_merged_reads"]
    assert st_d["n_reads_entered"] == st_h["n_reads_entered"]
    assert st_d["n_chunks"] >= sh.min_cut_chunks(group) and st_d["n_merged_reads"] > 0
    pu.assert_same_arrays(host, dev)
    sh.assert_matches_restatement(dev, group, K, b["info"])


@pytest.mark.parametrize("level", [0, 6])
@pytest.mark.parametrize("group,K", [c[:2] for c in sh.CUT_CASES])
def test_every_site_a_chunk(bams, group, K, level, monkeypatch):
    b = bams[level]
    monkeypatch.setenv("CTO_PHASE_CHUNK_BYTES", "1")
    host, dev, st_h, st_d = both(b["bam"], sh.case()["sites"][group], K)
    assert st_d["fallback_chunks"] == 0
    assert st_d["n_chunks"] == st_h["n_chunks"] == len(sh.case()["sites"][group])
    assert st_d["n_merged_reads"] == st_h["n_merged_reads"] > 0 and st_d["n_reads_entered"] == st_h["n_reads_entered"] > len(dev["voff"])
    pu.assert_same_arrays(host, dev)
    sh.assert_matches_restatement(dev, group, K, b["info"])


def test_a_damaged_chunk_goes_to_the_host_and_merges_with_the_rest(bams, monkeypatch):
    """one flipped bit in the CRC-32 of a BGZF block that holds q2's records only: every device chunk of q1 whose byte range reaches it
    is redone by the host path, which never opens it.  Without compression the file is longer than the 64 KiB a chunk reads on behind
    its last record, so the chunks of q1's first 16 kb stay on the device and both kinds merge into one result.  (At level 6 the whole
    file is shorter than that and every chunk would go to the host: no case for this test.)"""
    from clairs_to_amd.phase_tumor import phase_reads
    b = bams[0]
    sites = sh.case()["sites"]["all"]
    good = phase_reads(b["bam"], sh.CTG, *sh.sites_args("all"), where="host")
    monkeypatch.setenv("CTO_PHASE_CHUNK_BYTES", sh.CHUNK_BYTES)
    _, dev, st_h, st_d = both(b["bad"], sites)
    assert st_d["n_chunks"] == st_h["n_chunks"] >= sh.MIN_CUT_CHUNKS and 0 < st_d["fallback_chunks"] < st_d["n_chunks"]
    assert st_d["n_merged_reads"] == st_h["n_merged_reads"] > 0
    pu.assert_same_arrays(good, dev)
    _, clean, _, st_c = both(b["bam"], sites)                             # and the undamaged file stays on the device
    assert st_c["fallback_chunks"] == 0
    pu.assert_same_arrays(good, clean)


def test_no_sites(bams):
    host, dev, _, st_d = both(bams[6]["bam"], [])
    pu.assert_same_arrays(host, dev)
    assert len(dev["voff"]) == len(dev["phase"]) == len(dev["obs"]) == len(dev["hp"]) == 0 and list(dev["obs_off"]) == [0]
    assert dev["link"].shape == (0, 8, 2) and st_d["fallback_chunks"] == 0


@pytest.mark.parametrize("name", sorted(sh.small_ends()))
def test_small_ends(bams, name):
    b, sites = bams[6], sh.small_ends()[name]
    host, dev, st_h, st_d = both(b["bam"], sites, K=1)
    assert st_d["fallback_chunks"] == 0
    pu.assert_same_arrays(host, dev)
    assert st_d["n_phase_blocks"] == st_h["n_phase_blocks"] == len(sites)
    nv = pu.naive(sh.case()["reads"], 0, sites, K=1)
    got = pu.shaped(dev, 1)
    assert got["voff"] == [b["info"]["voff"][i] for i in nv["entered"]]
    for k in ("obs", "link", "phase", "ps", "tags"):
        assert got[k] == nv[k], k
    if name != "one_site":                                                # no read enters: the link table is all zero
        assert len(dev["voff"]) == 0 and not dev["link"].any() and list(dev["obs_off"]) == [0]


def test_buffers_are_reused_across_calls(bams):
    """the context's buffers grow and stay: the large case, the small one, the large one again"""
    b, c = bams[0], sh.case()
    _, big1, _, s1 = both(b["bam"], c["sites"]["all"], 64)
    host_small, small, _, s2 = both(b["bam"], c["sites"]["few"], 1)
    _, big2, _, s3 = both(b["bam"], c["sites"]["all"], 64)
    _, small2, _, s4 = both(b["bam"], c["sites"]["few"], 1)
    pu.assert_same_arrays(big1, big2)
    pu.assert_same_arrays(small, small2)
    pu.assert_same_arrays(host_small, small)
    sh.assert_matches_restatement(big2, "all", 64, b["info"])
    assert s1["fallback_chunks"] == s2["fallback_chunks"] == s3["fallback_chunks"] == s4["fallback_chunks"] == 0


def test_arguments_are_checked_on_the_device_path(bams):
    from clairs_to_amd._lib import CtoError
    from clairs_to_amd.phase_tumor import phase_reads
    pos, ref, alt = sh.sites_args("few")
    for where in ("host", "device"):
        with pytest.raises(CtoError, match="link_span must be 1 .. 64"):
            phase_reads(bams[6]["bam"], sh.CTG, pos, ref, alt, link_span=65, where=where)
        with pytest.raises(CtoError, match="strictly ascending"):
            phase_reads(bams[6]["bam"], sh.CTG, pos[::-1], ref, alt, where=where)
    st = {}                                                               # the largest link span there is passes the check
    at_64 = [phase_reads(bams[6]["bam"], sh.CTG, pos, ref, alt, link_span=64, where=w, stats=st if w == "device" else None) for w in ("host", "device")]
    assert st["fallback_chunks"] == 0 and at_64[1]["link"].shape == (3, 64, 2) and np.array_equal(at_64[0]["link"], at_64[1]["link"])
