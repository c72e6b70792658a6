"""The allele counter's host path (cto_allele_counts, where = 0) against the naive restatement of its rules in
tests/allelecountutil.py, exactly, and the bytes of the table the sub-command writes."""
import os

import numpy as np
import pytest

from allelecountutil import CHUNK_BYTES, PARAMS, REFS, case, expected, expected_table, loci_file_lines


def _count(ctg, params, where="host", **kw):
    from clairs_to_amd.allele_counter import count_alleles
    bq, mq, f, F = PARAMS[params]
    c = case()
    return count_alleles(c["bam"], ctg, c["loci"][ctg], min_bq=bq, min_mq=mq, req_flags=f, excl_flags=F, where=where, **kw)


@pytest.mark.parametrize("params", sorted(PARAMS))
@pytest.mark.parametrize("ctg", [n for n, _ in REFS])
def test_host_counts_equal_the_naive_rules(ctg, params):
    np.testing.assert_array_equal(_count(ctg, params), expected(ctg, params))


def test_the_case_holds_what_it_is_meant_to():
    """the host path on the generated BAM: the flag masks, MAPQ / BQ thresholds and mate rules change the counts they should"""
    c = case()
    at = lambda ctg, p: c["loci"][ctg].index(p)
    v, f0, f2 = _count("chrA", "verdict"), _count("chrA", "F0"), _count("chrA", "f2")
    assert f0[at("chrA", 950)].sum() == v[at("chrA", 950)].sum() + 2            # flags 8 and 2048 enter under -F 0; 4, 256, 512, 1024 never do
    assert f2[at("chrA", 1050)].sum() == 1 and f2[at("chrA", 1130)].sum() == 1  # the F/R pair only
    d = _count("chrA", "defaults")
    assert d[at("chrA", 1221)].sum() == 1 and d[at("chrA", 1321)].sum() == 2 and d[at("chrA", 1421)].sum() == 0
    assert d[at("chrA", 1521)].sum() == 0 and d[at("chrA", 1621)].sum() == 1
    assert _count("7", "verdict")[at("7", 3005)].sum() > 1024                 # deep: about three in four of 2100 reads pass BQ 20


def test_host_chunks_do_not_change_the_counts(monkeypatch):
    """a small chunk budget cuts chrA into several chunks, reads straddling every cut: the counts stay"""
    monkeypatch.setenv("CTO_ALLELE_CHUNK_BYTES", CHUNK_BYTES)
    c = case()
    stats = {}
    got = _count("chrA", "verdict", stats=stats, host_threads=3)
    assert stats["n_chunks"] >= 3 and stats["fallback_chunks"] == 0
    np.testing.assert_array_equal(got, expected("chrA", "verdict"))
    # every gap between neighbouring loci from 300 to 5600 lies inside some entered read: wherever the cuts are, reads straddle them
    loci = [p for p in c["loci"]["chrA"] if 300 <= p <= 5600]
    spans = [(r["pos"] + 1, r["pos"] + sum(n for op, n in r["cigar"] if op in "MDN=X")) for r in c["reads"] if r["ref"] == 0 and r["name"].startswith("long")]
    for a, b in zip(loci, loci[1:]):
        assert any(s <= a and b <= e for s, e in spans)


def test_bad_arguments_are_refused():
    from clairs_to_amd._lib import CtoError
    from clairs_to_amd.allele_counter import count_alleles
    c = case()
    with pytest.raises(CtoError):
        count_alleles(c["bam"], "chrA", [5, 5], where="host")                   # not strictly ascending
    with pytest.raises(CtoError):
        count_alleles(c["bam"], "chrZ", [5], where="host")                      # not in the header
    assert count_alleles(c["bam"], "chrA", [], where="host").shape == (0, 4)


def test_cli_writes_the_programs_table(tmp_path):
    from clairs_to_amd.__main__ import SUBMODULES, dispatch
    assert "allele_counter" in SUBMODULES
    loci_fn, out_fn = tmp_path / "loci.txt", tmp_path / "out.txt"
    loci_fn.write_text("\n".join(loci_file_lines()) + "\n")
    dispatch("allele_counter", ["-b", case()["bam"], "-l", str(loci_fn), "-o", str(out_fn), "-m", "20", "-q", "20", "-f", "0", "-F", "2316",
                                "--dense-snps", "--where", "host"])
    assert out_fn.read_text() == expected_table("verdict")


def test_cli_per_contig_convenience_and_refusals(tmp_path):
    from clairs_to_amd.allele_counter import main
    c = case()
    (tmp_path / "contigs").write_text("chrA\nchrUn\nchr1\n7\n")                 # only names among chr1..22, X are run: chr1
    loci = c["loci"]["chr1"]
    (tmp_path / "l_chr1.txt").write_text("".join("chr1\t%d\n" % p for p in loci[::-1]))
    main(["-b", c["bam"], "--contig_fn", str(tmp_path / "contigs"), "--loci_prefix", str(tmp_path / "l_"), "--output_prefix", str(tmp_path / "o_"),
          "-q", "20", "-f", "0", "-F", "2316", "--where", "host"])
    assert sorted(os.listdir(str(tmp_path))) == ["contigs", "l_chr1.txt", "o_chr1.txt"]
    want = "#CHR\tPOS\tCount_A\tCount_C\tCount_G\tCount_T\tGood_depth\n"
    want += "".join("chr1\t%d\t%d\t%d\t%d\t%d\t%d\n" % (p, *r, r.sum()) for p, r in zip(loci, expected("chr1", "verdict")))
    assert (tmp_path / "o_chr1.txt").read_text() == want
    with pytest.raises(SystemExit):
        main(["-b", c["bam"], "-l", "x", "-o", "y", "-x"])
    with pytest.raises(SystemExit):
        main(["-b", "tumor.cram", "-l", "x", "-o", "y"])
