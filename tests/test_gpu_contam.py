"""cto_bam_coverage and cto_bam_mix, device path (csrc/contam.hip) against the host path: the coverage tables equal, the output BAM and its
.bai byte for byte - integers only, so every comparison is exact - and no case may pass by falling back to the host.  What the host
path itself is held to: tests/test_gen_contaminated_bam.py."""
import os

import pytest

import bamutil
import contamutil as cu
import phaseutil as pu

pytestmark = pytest.mark.gpu

MIXES = [(500, 500, 0), (1000, 1000, 0), (700, 0, 3), (0, 1000, 7)]


def read(fn):
    with open(fn, "rb") as f:
        return f.read()


def coverage_both(bam, ctg=None):
    from clairs_to_amd.gen_contaminated_bam import bam_coverage
    st_h, st_d = {}, {}
    host = bam_coverage(bam, ctg, where="host", stats=st_h)
    dev = bam_coverage(bam, ctg, where="device", stats=st_d)
    assert st_d["fallback_chunks"] == 0
    return host, dev, st_h, st_d


def mix_both(b, d, tag, m_t, m_n, seed, ctg=None, threads=2):
    from clairs_to_amd.gen_contaminated_bam import mix_bams
    st_h, st_d = {}, {}
    out_h, out_d = str(d / ("%s_host.bam" % tag)), str(d / ("%s_dev.bam" % tag))
    res_h = mix_bams(b["t"], b["n"], out_h, m_t, m_n, seed=seed, ctg=ctg, where="host", host_threads=threads, stats=st_h)
    res_d = mix_bams(b["t"], b["n"], out_d, m_t, m_n, seed=seed, ctg=ctg, where="device", host_threads=threads, stats=st_d)
    assert st_d["fallback_chunks"] == 0
    assert res_h == res_d
    return out_h, out_d, st_h, st_d


@pytest.fixture(scope="module")
def bams(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_contam")
    out = {"dir": d}
    sims = {s: pu.sim_case(s) for s in (7, 11)}
    for level in (0, 6):
        cov = str(d / ("cov_l%d.bam" % level))
        bamutil.write_bam(cov, cu.HAND_REFS, cu.coverage_reads(), block_payload=3000, level=level)
        t, n = str(d / ("t_l%d.bam" % level)), str(d / ("n_l%d.bam" % level))
        bamutil.write_bam(t, cu.HAND_REFS, cu.mix_reads("t"), block_payload=3000, level=level)
        bamutil.write_bam(n, cu.HAND_REFS, cu.mix_reads("n"), block_payload=3000, level=level)
        out["hand", level] = dict(cov=cov, t=t, n=n)
        st, sn = str(d / ("sim7_l%d.bam" % level)), str(d / ("sim11_l%d.bam" % level))
        refs = [(pu.SIM_CTG, sims[7]["ref_len"])]
        bamutil.write_bam(st, refs, sims[7]["reads"], level=level)
        bamutil.write_bam(sn, refs, [dict(r, name="n" + r["name"]) for r in sims[11]["reads"]], level=level)     # names of its own: keys of its own
        out["sim", level] = dict(cov=st, t=st, n=sn)
    return out


@pytest.mark.parametrize("level", [0, 6])
@pytest.mark.parametrize("which", ["hand", "sim"])
def test_coverage_device_equals_host(bams, which, level):
    b = bams[which, level]
    host, dev, st_h, st_d = coverage_both(b["cov"])
    assert dev == host
    assert st_d["n_blocks"] > 0 and st_d["inflated_bytes"] > 0 and st_d["n_records"] == st_h["n_records"] > 10
    if which == "hand":
        assert dev == cu.coverage_table(b["cov"])
        for ctg in ("c1", "c3"):
            h1, d1, _, _ = coverage_both(b["cov"], ctg)
            assert d1 == h1 == [r for r in host if r["chrom"] == ctg]
    other = bams[which, level]["n"]
    host, dev, _, _ = coverage_both(other)
    assert dev == host


@pytest.mark.parametrize("level", [0, 6])
@pytest.mark.parametrize("which", ["hand", "sim"])
def test_mix_device_equals_host(bams, which, level):
    b = bams[which, level]
    for m_t, m_n, seed in MIXES:
        out_h, out_d, st_h, st_d = mix_both(b, bams["dir"], "%s%d_%d_%d_%d" % (which, level, m_t, m_n, seed), m_t, m_n, seed)
        assert read(out_d) == read(out_h) and read(out_d + ".bai") == read(out_h + ".bai")
        assert st_d["n_blocks"] > 0 and st_d["out_bytes"] == st_h["out_bytes"] > 0
        assert st_d["kept"] == st_h["kept"] and st_d["candidates"] == st_h["candidates"]
    if which == "hand":
        out_h, out_d, _, _ = mix_both(b, bams["dir"], "hand%d_c1" % level, 400, 600, 1, ctg="c1")
        assert read(out_d) == read(out_h) and read(out_d + ".bai") == read(out_h + ".bai")


@pytest.mark.parametrize("level", [0, 6])
def test_several_windows_give_the_same_files_and_tables(bams, level, monkeypatch):
    """the hand-built BAMs hold a read over more than two 16 kb windows (its end is carried twice) and equal positions on both sides of
    a window edge, in both the coverage and the mix input"""
    b = bams["hand", level]
    cov_one, cov_dev_one, _, st_one = coverage_both(b["cov"])
    assert st_one["n_chunks"] == 3                                                         # one window per contig
    one_h, one_d, _, st_mix_one = mix_both(b, bams["dir"], "w1_%d" % level, 600, 400, 2)
    assert st_mix_one["n_chunks"] == 3
    for budget, least in (("20000", 4), ("1", 10)):
        monkeypatch.setenv("CTO_CONTAM_CHUNK_BYTES", budget)
        host, dev, st_h, st_d = coverage_both(b["cov"])
        assert st_d["n_chunks"] >= least and st_d["n_chunks"] == st_h["n_chunks"]
        assert dev == host == cov_one
        cut_h, cut_d, st_h, st_d = mix_both(b, bams["dir"], "w%s_%d" % (budget, level), 600, 400, 2)
        assert st_d["n_chunks"] >= least and st_d["n_chunks"] == st_h["n_chunks"]
        if budget == "1":
            assert st_d["n_chunks"] == 7 + 2 + 1                                           # every 16 kb window is its own chunk
        assert read(cut_d) == read(one_d) == read(cut_h) == read(one_h)
        assert read(cut_d + ".bai") == read(one_d + ".bai") == read(cut_h + ".bai")


def test_device_output_against_the_restatement(bams):
    b = bams["hand", 6]
    out_h, out_d, _, _ = mix_both(b, bams["dir"], "restated", 500, 500, 0)
    header, refs, t_recs = cu.read_bam(b["t"])
    _, _, n_recs = cu.read_bam(b["n"])
    merged = cu.merged_records(t_recs, n_recs, len(refs), 500, 500, 0)
    stream, eof = cu.inflated(out_d)
    assert eof and stream == cu.stream_of(header, merged)
    assert read(out_d + ".bai") == cu.expected_bai(out_d, header, len(refs), merged)


def test_cli_device_writes_what_the_cli_host_writes(bams, capsys):
    from clairs_to_amd.gen_contaminated_bam import main
    b = bams["hand", 6]
    outs = {}
    for where in ("host", "device"):
        od = str(bams["dir"] / ("cli_" + where))
        main(["--tumor_bam_fn", b["t"], "--normal_bam_fn", b["n"], "--output_dir", od, "--tumor_purity", "0.7", "--cal_output_bam_coverage", "1",
              "--where", where, "--samtools_threads", "3"])
        printed = capsys.readouterr().out.replace(od, "OUT")
        files = sorted(os.path.join(dp, f)[len(od):] for dp, _, fs in os.walk(od) for f in fs)
        outs[where] = (printed, files, [read(od + f) for f in files])
    assert outs["device"] == outs["host"]
    assert outs["device"][1] == ["/cov.cov.mosdepth.summary.txt", "/tmp/raw_normal.cov.mosdepth.summary.txt", "/tmp/raw_tumor.cov.mosdepth.summary.txt",
                                 "/tumor_purity_0.7.bam", "/tumor_purity_0.7.bam.bai"]
