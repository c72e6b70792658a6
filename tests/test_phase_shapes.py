"""cto_phase_reads, host path (csrc/bam.cpp), on the BAM of tests/phaseshapes.py: reads of more than 64 and 128 CIGAR operations, more than
64 sites under one operation, reads of more than 64 observations, link spans up to the limit, more than 70 phase blocks with ties and
threshold votes - against the naive restatement (tests/phaseutil.py) and against the planted facts written out by hand.  Building the
case runs phaseshapes.check_case, so an input that lost one of its edges fails here.  tests/test_gpu_phase_shapes.py holds the device
path to the same.  No GPU."""
import pytest

import phaseshapes as sh
import phaseutil as pu

from clairs_to_amd.phase_tumor import phase_reads

CASES = [(g, K) for g in sh.GROUPS + ("all",) for K in sh.LINK_SPANS]


@pytest.fixture(scope="module")
def bams(tmp_path_factory):
    d = tmp_path_factory.mktemp("phase_shapes")
    out = {}
    for level in (0, 6):
        bam = d / ("l%d.bam" % level)
        out[level] = dict(bam=str(bam), info=sh.write(bam, level=level), dir=d)
    return out


def host(b, group, K, **kw):
    return phase_reads(b["bam"], sh.CTG, *sh.sites_args(group), link_span=K, where="host", **kw)


def test_the_case_holds_its_edges():
    c = sh.case()                                          # check_case: operation indices, observation counts, blocks, votes
    assert max(len(r["cigar"]) for r in c["reads"]) == 362 and len(c["sites"]["all"]) > 500
    assert all(sh.expected("blocks", K)["n_blocks"] >= 70 for K in sh.LINK_SPANS)


def test_records_straddle_blocks(bams):
    info = bams[6]["info"]
    assert max(info["block_sizes"]) == sh.BLOCK_PAYLOAD and len(info["block_sizes"]) > 200
    starts = {0}
    for s in info["block_sizes"]:
        starts.add(max(starts) + s)
    cut = [any(a < x < b for x in starts) for a, b in info["record_spans"]]
    assert sum(cut) > 0.5 * len(cut) and cut[sh.case()["by_name"]["ops362"]] and cut[sh.case()["by_name"]["ops150cg"]]


@pytest.mark.parametrize("group,K", CASES)
def test_host_against_the_restatement(bams, group, K):
    stats = {}
    got = sh.assert_matches_restatement(host(bams[6], group, K, stats=stats), group, K, bams[6]["info"])
    sh.assert_by_hand(got, group, K, bams[6]["info"])
    assert stats["n_phase_blocks"] == sh.expected(group, K)["n_blocks"]


def test_level_0_is_the_same_reads(bams):
    for group, K in (("all", 8), ("ops", 64)):
        sh.assert_matches_restatement(host(bams[0], group, K), group, K, bams[0]["info"])


@pytest.mark.parametrize("level", [0, 6])
@pytest.mark.parametrize("group,K,budget", sh.CUT_CASES)
def test_chunks_change_nothing(bams, group, K, budget, level, monkeypatch):
    b = bams[level]
    monkeypatch.delenv("CTO_PHASE_CHUNK_BYTES", raising=False)
    one = host(b, group, K, host_threads=1)
    monkeypatch.setenv("CTO_PHASE_CHUNK_BYTES", budget)
    st = {}
    cut = host(b, group, K, host_threads=3, stats=st)
    assert st["n_chunks"] >= sh.min_cut_chunks(group) and st["n_merged_reads"] > 0
    pu.assert_same_arrays(one, cut)
    monkeypatch.setenv("CTO_PHASE_CHUNK_BYTES", "1")                      # every site a chunk of its own
    st = {}
    each = host(b, group, K, stats=st)
    assert st["n_chunks"] == len(sh.case()["sites"][group]) and st["n_merged_reads"] > 0
    assert st["n_reads_entered"] > len(each["voff"])
    pu.assert_same_arrays(one, each)
    sh.assert_matches_restatement(each, group, K, b["info"])


def test_the_host_path_never_opens_the_damaged_block(bams, tmp_path, monkeypatch):
    b = bams[6]
    sh.write_damaged(b["bam"], tmp_path / "bad.bam", b["info"])
    assert open(b["bam"], "rb").read() != open(str(tmp_path / "bad.bam"), "rb").read()
    good = host(b, "all", 8)
    pu.assert_same_arrays(good, phase_reads(str(tmp_path / "bad.bam"), sh.CTG, *sh.sites_args("all"), where="host"))
    monkeypatch.setenv("CTO_PHASE_CHUNK_BYTES", sh.CHUNK_BYTES)
    pu.assert_same_arrays(good, phase_reads(str(tmp_path / "bad.bam"), sh.CTG, *sh.sites_args("all"), where="host"))
    from clairs_to_amd._lib import CtoError
    with pytest.raises(CtoError):                                         # q2's own reads do run into it
        phase_reads(str(tmp_path / "bad.bam"), sh.CTG2, [150, 900], "AA", "CC", where="host")


def test_small_ends(bams):
    c, b = sh.case(), bams[6]
    for name, sites in sh.small_ends().items():
        args = [s[0] for s in sites], [s[1] for s in sites], [s[2] for s in sites]
        st = {}
        got = pu.shaped(phase_reads(b["bam"], sh.CTG, *args, link_span=1, where="host", stats=st), 1)
        nv = pu.naive(c["reads"], 0, sites, K=1)
        assert got["voff"] == [b["info"]["voff"][i] for i in nv["entered"]]
        for k in ("obs", "link", "phase", "ps", "tags"):
            assert got[k] == nv[k], (name, k)
        assert st["n_phase_blocks"] == len(sites)
        assert (len(got["voff"]) > 5) == (name == "one_site") and (name == "one_site" or (got["voff"] == [] and got["link"] == {}))
