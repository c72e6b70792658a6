"""gen_contaminated_bam, host path (csrc/bam.cpp): cto_bam_coverage, cto_bam_mix and the keep rule against the rules restated naively
(tests/contamutil.py) on BAMs built by hand, the command line against what the reference prints under --dry_run
(tests/golden/contam_dry_run.json.gz), and one run end to end.  PARITY UNPINNED against mosdepth and samtools: the rules are the
definition (csrc/contam.hip).  No GPU."""
import math
import os

import pytest

import bamutil
import contamutil as cu
from conftest import load_json_gz

from clairs_to_amd._lib import CtoError
from clairs_to_amd.gen_contaminated_bam import bam_coverage, build_parser, main, mix_bams, subsample_keys
from clairs_to_amd.realign_reads import bam_view

# the issue's known answers: name, k & 0xffffff at seed 0 and at seed 7 (computed from the rule on the CPU, not by samtools)
KNOWN = [("r0", 4933748, 16244436), ("read_17", 3974049, 1362500), ("m64011_190830_220126/1/ccs", 12273429, 7464176), ("a", 9126454, 4231483),
         ("SRR1.1000000", 11214744, 6228894)]


# ------------------------------------------------------------------------------------------ rule b
def test_hash_known_answers():
    names = [k[0] for k in KNOWN]
    assert [int(x) for x in subsample_keys(names, seed=0)[0]] == [k[1] for k in KNOWN]
    assert [int(x) for x in subsample_keys(names, seed=7)[0]] == [k[2] for k in KNOWN]
    assert [cu.key24(n.encode(), 0) for n in names] == [k[1] for k in KNOWN]            # the restatement is the same rule
    assert int(subsample_keys([""], seed=0)[0][0]) == cu.key24(b"", 0)                   # the empty name: h = 0


def test_names_of_length_1_and_254_and_high_bytes():
    names = [b"x", b"q" * 254, bytes(range(1, 255)), b"\xff\xfe", b"ab"]
    for seed in (0, 7, 0xffffffff):
        assert [int(x) for x in subsample_keys(names, seed=seed)[0]] == [cu.key24(n, seed) for n in names]
    with pytest.raises(CtoError):
        subsample_keys([b"z" * 255])


@pytest.mark.parametrize("m", [0, 1, 125, 500, 999, 1000])
def test_keep_against_the_restatement(m):
    names = ["read/%d/ccs" % (i * 7919) for i in range(4000)]
    for seed in (0, 11):
        k24, keep = subsample_keys(names, seed=seed, m=m)
        want = [cu.keeps(cu.key24(n.encode(), seed), m) for n in names]
        assert [bool(x) for x in keep] == want
        if m == 0:
            assert not any(want)
        if m == 1000:
            assert all(want)
        if m == 500:
            assert abs(sum(want) - 2000) < 5 * math.sqrt(4000 * 0.25)                    # the hash spreads the names


# ------------------------------------------------------------------------------------------ rule a
@pytest.fixture(scope="module")
def cov_bam(tmp_path_factory):
    bam = str(tmp_path_factory.mktemp("contam_cov") / "cov.bam")
    bamutil.write_bam(bam, cu.HAND_REFS, cu.coverage_reads(), block_payload=3000)
    return bam


def test_coverage_against_the_depth_array(cov_bam):
    want = cu.coverage_table(cov_bam)
    stats = {}
    assert bam_coverage(cov_bam, where="host", stats=stats) == want
    by = {r["chrom"]: r for r in want}
    assert by["c2"] == dict(chrom="c2", length=30000, bases=0, min=0, max=0)            # a contig with no reads
    assert by["c3"]["min"] == 2 and by["c3"]["max"] == 3 and by["c3"]["bases"] == 1100   # covered everywhere; full2 is clipped at 500
    assert by["c1"]["min"] == 0 and by["c1"]["max"] >= 3
    assert stats["fallback_chunks"] == 0 and stats["n_chunks"] >= 3
    # what the excluded records and the special ones would have added, had they counted otherwise
    _, _, recs = cu.read_bam(cov_bam)
    d = cu.depth_array(recs, 0, 100000)
    assert d[2550] == 0 and d[2650] == 0 and d[2750] == 0 and d[2850] == 0 and d[2950] == 1 and d[3050] == 1       # the four flags; 2048; MAPQ 0
    assert d[1549] == 1 and d[1550] == 0                                                 # the CG tag's CIGAR: 550 reference bases from 1000
    assert d[2000] == 0                                                                  # rlen == 0
    assert d[99999] == 1 and sum(d[99800:]) == 200                                       # clipped at the contig's end
    for ctg in ("c1", "c2", "c3"):
        assert bam_coverage(cov_bam, ctg, where="host") == [by[ctg]]


def test_coverage_does_not_depend_on_the_windows(cov_bam, monkeypatch):
    want = bam_coverage(cov_bam, where="host")
    for budget in ("1", "70000", "100000000"):
        monkeypatch.setenv("CTO_CONTAM_CHUNK_BYTES", budget)
        stats = {}
        assert bam_coverage(cov_bam, where="host", stats=stats) == want, budget
        if budget == "1":
            assert stats["n_chunks"] == 7 + 2 + 1                                        # every 16 kb window is its own chunk
        if budget == "100000000":
            assert stats["n_chunks"] == 3


def test_coverage_errors(cov_bam, tmp_path):
    with pytest.raises(CtoError, match="not in the BAM header"):
        bam_coverage(cov_bam, "c9", where="host")
    with pytest.raises(CtoError, match="cannot open index"):
        bam_coverage(cov_bam, where="host", bai=str(tmp_path / "none.bai"))


# ------------------------------------------------------------------------------------------ rules c and d
@pytest.fixture(scope="module", params=[0, 6], ids=["stored", "level6"])
def mix_pair(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("contam_mix%d" % request.param)
    t, n = str(d / "t.bam"), str(d / "n.bam")
    bamutil.write_bam(t, cu.HAND_REFS, cu.mix_reads("t"), block_payload=3000, level=request.param)
    bamutil.write_bam(n, cu.HAND_REFS, cu.mix_reads("n"), block_payload=3000, level=request.param)
    header, refs, t_recs = cu.read_bam(t)
    _, _, n_recs = cu.read_bam(n)
    assert max(len(r) for r in t_recs) > 65536                                           # one record above 64 KB
    return dict(dir=d, t=t, n=n, header=header, refs=refs, t_recs=t_recs, n_recs=n_recs)


def check_mix(p, out, m_t, m_n, seed, ctg, res):
    only = None if ctg is None else [n for n, _ in p["refs"]].index(ctg)
    merged = cu.merged_records(p["t_recs"], p["n_recs"], len(p["refs"]), m_t, m_n, seed, only)
    stream, eof = cu.inflated(out)
    assert eof
    assert stream[:len(p["header"])] == p["header"]                                      # the tumour's header, verbatim
    assert stream == cu.stream_of(p["header"], merged)
    sizes = cu.block_sizes(out)
    assert all(s == 0xff00 for s in sizes[:-2]) and sizes[-1] == 0 and 0 < sizes[-2] <= 0xff00
    cand = [sum(1 for r in recs if (only is None or cu.fields(r)["tid"] == only) and cu.fields(r)["pos"] >= 0) for recs in (p["t_recs"], p["n_recs"])]
    assert res["candidates"] == cand
    assert sum(res["kept"]) == len(merged)
    # the index, by the rules of haplotag_bam over the blocks the file has
    assert open(str(out) + ".bai", "rb").read() == cu.expected_bai(out, p["header"], len(p["refs"]), merged)
    want = str(out) + ".want.bam"
    cu.write_expected(want, p["header"], len(p["refs"]), merged)
    if os.path.getsize(want) == os.path.getsize(out):                                    # the same zlib in Python and the library: the same files
        assert open(want, "rb").read() == open(out, "rb").read()
        assert open(want + ".bai", "rb").read() == open(str(out) + ".bai", "rb").read()
    for c, s, e in (("c1", 1, 100000), ("c1", 700, 800), ("c1", 16384, 16385), ("c1", 3500, 3600), ("c1", 50000, 66000), ("c2", 1, 30000),
                    ("c3", 1, 500), ("c1", 72990, 73010)):
        if ctg is not None and c != ctg:
            continue
        assert bam_view(out, c, s, e) == cu.view_rows(merged, p["refs"], c, s, e), (c, s, e)
    return merged


@pytest.mark.parametrize("m_t,m_n,seed,ctg", [(500, 500, 0, None), (1000, 1000, 0, None), (800, 0, 3, None), (0, 400, 0, "c1"), (250, 1000, 7, "c1"),
                                              (1000, 500, 0, "c3"), (0, 0, 0, None)])
def test_mix_against_the_restatement(mix_pair, m_t, m_n, seed, ctg):
    p = mix_pair
    out = str(p["dir"] / ("out_%d_%d_%d_%s.bam" % (m_t, m_n, seed, ctg)))
    stats = {}
    res = mix_bams(p["t"], p["n"], out, m_t, m_n, seed=seed, ctg=ctg, where="host", stats=stats)
    merged = check_mix(p, out, m_t, m_n, seed, ctg, res)
    assert stats["fallback_chunks"] == 0
    if (m_t, m_n) == (1000, 1000) and ctg is None:
        assert len(merged) == len(p["t_recs"]) + len(p["n_recs"])
        names = [cu.fields(r)["name"] for _, r in merged]
        i = names.index(b"ttie3")                                                         # ties at 16384: the tumour's two, then the normal's
        assert names[i:i + 4] == [b"ttie3", b"ttie4", b"ntie3", b"ntie4"]
    if m_n == 0:
        assert res["kept"][1] == 0                                                        # a source with nothing kept
    names = [cu.fields(r)["name"] for _, r in merged]
    assert names.count(b"tmate") in (0, 2) and names.count(b"nmate") in (0, 2)             # pairs stay together


def test_mix_bytes_do_not_depend_on_threads_or_windows(mix_pair, monkeypatch):
    p = mix_pair
    outs = []
    for k, (threads, budget) in enumerate(((1, None), (4, None), (4, "1"), (1, "60000"))):
        if budget:
            monkeypatch.setenv("CTO_CONTAM_CHUNK_BYTES", budget)
        out = str(p["dir"] / ("thr_%d.bam" % k))
        stats = {}
        mix_bams(p["t"], p["n"], out, 700, 300, seed=1, where="host", host_threads=threads, stats=stats)
        outs.append((open(out, "rb").read(), open(out + ".bai", "rb").read()))
        if budget == "1":
            assert stats["n_chunks"] == 7 + 2 + 1
    assert all(o == outs[0] for o in outs[1:])


def test_mix_errors(mix_pair, tmp_path):
    p = mix_pair
    out = str(tmp_path / "o.bam")
    # an unsorted source
    reads = cu.mix_reads("n")
    k = next(i for i in range(1, len(reads)) if reads[i]["ref"] == 0 and reads[i - 1]["ref"] == 0 and reads[i]["pos"] > reads[i - 1]["pos"] and
             reads[i]["pos"] >> 14 == reads[i - 1]["pos"] >> 14 and reads[i]["pos"] > 20000)
    reads[k - 1], reads[k] = reads[k], reads[k - 1]
    bad = str(tmp_path / "unsorted.bam")
    bamutil.write_bam(bad, cu.HAND_REFS, reads)
    with pytest.raises(CtoError, match="not coordinate-sorted"):
        mix_bams(p["t"], bad, out, 1000, 1000, where="host")
    with pytest.raises(CtoError, match="not coordinate-sorted"):
        mix_bams(bad, p["n"], out, 1000, 1000, where="host")
    # differing reference lists: count, name, length
    for refs, what in (([("c1", 100000), ("c2", 30000)], "3 references"), ([("c1", 100000), ("cX", 30000), ("c3", 500)], "reference 1 is c2"),
                       ([("c1", 100000), ("c2", 30001), ("c3", 500)], "c2 has length 30000")):
        other = str(tmp_path / "other.bam")
        bamutil.write_bam(other, refs, [cu.rd("x", 0, 5, [("M", 10)])])
        with pytest.raises(CtoError, match=what):
            mix_bams(p["t"], other, out, 1000, 1000, where="host")
    # a missing index is an error, of either source
    with pytest.raises(CtoError, match="cannot open index"):
        mix_bams(p["t"], p["n"], out, 1000, 1000, where="host", normal_bai=str(tmp_path / "none.bai"))
    with pytest.raises(CtoError, match="cannot open index"):
        mix_bams(p["t"], p["n"], out, 1000, 1000, where="host", tumor_bai=str(tmp_path / "none.bai"))
    with pytest.raises(CtoError, match="thousandths"):
        mix_bams(p["t"], p["n"], out, 1001, 0, where="host")


# ------------------------------------------------------------------------------------------ the command line
def test_parser_takes_the_reference_options():
    gold = load_json_gz("contam_dry_run.json.gz")
    mine = {o: a for a in build_parser()._actions for o in a.option_strings}
    for opt in gold["parser"]:
        for o in opt["options"]:
            assert o in mine, o
            if opt["action"] == "_StoreTrueAction":
                assert type(mine[o]).__name__ == "_StoreTrueAction"
    from clairs_to_amd.__main__ import SUBMODULES
    assert "gen_contaminated_bam" in SUBMODULES


def test_dry_run_prints_the_reference_lines(capsys, tmp_path, monkeypatch):
    gold = load_json_gz("contam_dry_run.json.gz")
    monkeypatch.chdir(tmp_path)
    assert len(gold["cases"]) >= 12
    for c in gold["cases"]:
        main(c["argv"])
        assert capsys.readouterr().out.split("\n")[:-1] == c["lines"], c["name"]
    assert os.listdir(str(tmp_path)) == []                                                # nothing is written


def test_end_to_end(tmp_path, capsys):
    """3000 tumour and 3000 normal reads of 500 bases on one contig of 100 kb: 15x each.  At purity 0.6 the reference's arithmetic keeps
    m_t = 600 and m_n = 400 thousandths.  Every read has the same length and lies wholly inside the contig, so the output's coverage is
    500 * (K_t + K_n) / 100000 with K binomial: its standard deviation is 500 * sqrt(3000 * 0.6 * 0.4 + 3000 * 0.4 * 0.6) / 100000 = 0.19.
    The bound is five of them, plus 0.005 for each of the three means being printed with two decimals."""
    n, length, read_len, purity = 3000, 100000, 500, 0.6
    t, nb, od = str(tmp_path / "t.bam"), str(tmp_path / "n.bam"), str(tmp_path / "out")
    bamutil.write_bam(t, [("chrT", length)], cu.uniform_reads("t", n, length, read_len, 1), block_payload=30000)
    bamutil.write_bam(nb, [("chrT", length)], cu.uniform_reads("n", n, length, read_len, 2), block_payload=30000)
    main(["--tumor_bam_fn", t, "--normal_bam_fn", nb, "--output_dir", od, "--tumor_purity", str(purity), "--cal_output_bam_coverage", "1", "--where", "host",
          "--samtools_threads", "64", "--samtools", "/nowhere/samtools"])
    lines = capsys.readouterr().out.split("\n")
    assert lines[0] == "[INFO] Normal/Tumor BAM coverage: 15.0/15.0"
    assert lines[1] == "[INFO] Normal/Tumor subsample proportion: 0.400/0.600"
    assert lines[-2] == "[INFO] Finishing merging, output file: %s/tumor_purity_0.6.bam" % od
    out = os.path.join(od, "tumor_purity_0.6.bam")
    for fn in (out, out + ".bai", os.path.join(od, "tmp", "raw_normal.cov.mosdepth.summary.txt"), os.path.join(od, "tmp", "raw_tumor.cov.mosdepth.summary.txt"),
               os.path.join(od, "cov.cov.mosdepth.summary.txt")):
        assert os.path.exists(fn), fn
    rows = [ln.split("\t") for ln in open(os.path.join(od, "cov.cov.mosdepth.summary.txt")).read().split("\n")[:-1]]
    assert rows[0] == ["chrom", "length", "bases", "mean", "min", "max"] and rows[1][0] == "chrT" and rows[2][0] == "total" and len(rows) == 3
    assert rows[1][1:] == rows[2][1:] and rows[1][3] == "%.2f" % (int(rows[1][2]) / length)
    got = float(rows[2][3])
    sd = read_len * math.sqrt(n * 0.6 * 0.4 + n * 0.4 * 0.6) / length
    assert abs(got - 15.0) <= 5 * sd + 0.015, (got, sd)
    assert cu.coverage_table(out) == [dict(chrom="chrT", length=length, bases=int(rows[1][2]), min=int(rows[1][4]), max=int(rows[1][5]))]
    # --remove_intermediate_dir removes tmp/ (the reference raises an AttributeError there)
    main(["--tumor_bam_fn", t, "--normal_bam_fn", nb, "--output_dir", od, "--tumor_purity", str(purity), "--where", "host", "--normal_bam_coverage", "15",
          "--tumor_bam_coverage", "15", "--remove_intermediate_dir"])
    assert not os.path.exists(os.path.join(od, "tmp")) and os.path.exists(out)
