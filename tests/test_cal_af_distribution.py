"""cal_af_distribution on the host path against the reference's own output (tests/golden/cal_af.json.gz: src/cal_af_distribution.py run
on the case of tests/calafutil.py, its samtools a stand-in that prints calafutil's rows), byte for byte, and against the naive rules of
calafutil.py; the parser against the reference's option table; the HP:i:12 error."""
import json

import numpy as np
import pytest

import calafutil
from bamutil import write_bam

GOLDEN = calafutil.golden()
CONFIGS = {c["name"]: c for c in GOLDEN["configs"]}
VALUE = {"int": "3", "str": "x", "str2bool": "False"}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("cal_af"))
    calafutil.write_vcfs(d)
    return d


def test_the_case_is_the_one_the_fixture_was_made_from():
    c = calafutil.case()
    assert GOLDEN["seed"] == calafutil.SEED and GOLDEN["n_reads"] == len(c["reads"]) and GOLDEN["reads_sha256"] == calafutil.reads_digest(c["reads"])
    assert calafutil.vcf_texts() == (GOLDEN["truth_vcf"], GOLDEN["input_vcf"])
    for key, row in GOLDEN["rows"].items():
        ctg, pos, hp = key.rsplit(":", 2)
        assert calafutil.mpileup_row(c["entered"][ctg], ctg, int(pos), hp == "1") == row, key


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_host_path_writes_the_references_file(files, tmp_path, name):
    from clairs_to_amd.__main__ import SUBMODULES, dispatch
    assert "cal_af_distribution" in SUBMODULES
    out = tmp_path / "out.txt"
    dispatch("cal_af_distribution", calafutil.config_argv(CONFIGS[name], files, out, "host"))
    assert out.read_bytes() == CONFIGS[name]["output"].encode()


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_host_path_returns_the_references_dict(files, name):
    from clairs_to_amd.cal_af_distribution import build_parser, cal_af
    got = cal_af(build_parser().parse_args(calafutil.config_argv(CONFIGS[name], files, None, "host")))
    pairs = json.loads(json.dumps([[k, v] for k, v in got.items()]))         # tuples -> lists, as the fixture stores them
    assert pairs == CONFIGS[name]["returned"]
    assert all(isinstance(k, tuple) and isinstance(v, tuple) for k, v in got.items() if len(v) == 6)


def test_input_vcf_rows_come_first(files, tmp_path):
    from clairs_to_amd.cal_af_distribution import main
    out = tmp_path / "out.txt"
    main(calafutil.config_argv(CONFIGS["all_hp"], files, out, "host"))
    widths = [len(ln.split(" ")) for ln in out.read_text().splitlines()]
    n4 = widths.count(4)
    assert n4 > 10 and widths == [4] * n4 + [10] * (len(widths) - n4)
    assert "chrA 5999 30 15\n" not in out.read_text()              # a call of the input VCF that is no truth variant


def test_parser_takes_every_option_of_the_reference():
    from clairs_to_amd.cal_af_distribution import build_parser
    table = GOLDEN["parser"]
    assert len(table) == 13
    everything = []
    for row in table:
        assert row["action"] == "_StoreAction" and row["nargs"] is None and not row["required"], row
        one = [row["options"][0], VALUE[row["type"]]]
        build_parser().parse_args(one)
        with pytest.raises(SystemExit):
            build_parser().parse_args(one[:1])                    # the reference's arity: one value
        everything += one
    a = build_parser().parse_args(everything)
    assert a.threads == 3 and a.phase_output is False and a.ctg_name == "x"
    d = build_parser().parse_args([])
    for row in table:
        name = row["options"][0][2:]
        if name not in ("samtools", "min_mq", "min_bq", "min_bq_cut"):         # accepted, never read
            assert getattr(d, name) == row["default"], row


@pytest.mark.parametrize("ctg", [n for n, _ in calafutil.REFS])
@pytest.mark.parametrize("with_hp", [True, False])
@pytest.mark.parametrize("max_depth", [8000, calafutil.LOW_MAX_DEPTH])
def test_host_tallies_equal_the_naive_rules(ctg, with_hp, max_depth):
    from clairs_to_amd.cal_af_distribution import allele_of, tally
    loci, ra = calafutil.contig_loci(ctg)
    got = tally(calafutil.case()["bam"], ctg, loci, [allele_of(r, a) for r, a in ra], with_hp=with_hp, max_depth=max_depth, where="host", host_threads=3)
    np.testing.assert_array_equal(got, calafutil.expected(ctg, with_hp, max_depth))


def test_alleles():
    from clairs_to_amd.cal_af_distribution import KIND_DEL, KIND_INS, KIND_NEVER, KIND_SNV, allele_of
    assert allele_of("A", "c") == (KIND_SNV, "C", 0, b"")
    assert allele_of("A", "Agat") == (KIND_INS, "A", 0, b"GAT")
    assert allele_of("gTT", "G") == (KIND_DEL, "G", 2, b"")
    for ref, alt in (("AT", "GC"), ("A", "<DEL>"), ("A", "R"), ("A", ""), ("AT", "R")):
        assert allele_of(ref, alt)[0] == (KIND_DEL if (ref, alt) == ("AT", "R") else KIND_NEVER)


def _hp12_bam(tmp_path):
    hp = calafutil.hp_aux
    rd = lambda name, pos, cigar, aux: dict(name=name, flag=0, ref=0, pos=pos, mapq=60, cigar=cigar, qual=[30] * 30,
                                            seq="C" * sum(n for op, n in cigar if op in "MIS"), aux=aux)
    reads = [rd("one", 0, [("M", 30)], hp("C", 1)), rd("twelve", 2, [("M", 30)], hp("s", 12, "ZB")), rd("none", 4, [("M", 30)], hp(None, 0)),
             rd("skip", 40, [("M", 5), ("N", 20), ("M", 5)], hp("C", 1)), rd("two", 42, [("M", 30)], hp("C", 2)), rd("twelve_last", 44, [("M", 30)], hp("i", 12))]
    for r in reads:
        r["qual"] = [30] * len(r["seq"])
    bam = str(tmp_path / "hp12.bam")
    write_bam(bam, [("c", 200)], reads, block_payload=700)
    return bam, calafutil.entered(reads, 0)


def test_hp_12_ends_the_run_as_the_reference_raises(tmp_path):
    from clairs_to_amd._lib import CtoError
    from clairs_to_amd.cal_af_distribution import allele_of, main, tally
    bam, ent = _hp12_bam(tmp_path)
    with pytest.raises(IndexError):
        calafutil.naive_tally(ent, "c", 10, "A", "C", True)
    with pytest.raises(CtoError, match="c:10 is paired with HP:i:12"):
        tally(bam, "c", [10], [allele_of("A", "C")], where="host")
    # without the HP column nothing is paired; behind a reference skip the entries take the values of the covers in front of them and
    # the last cover's 12 is dropped: no error, as in the reference
    np.testing.assert_array_equal(tally(bam, "c", [10], [allele_of("A", "C")], with_hp=False, where="host"), [calafutil.naive_tally(ent, "c", 10, "A", "C", False)])
    want = calafutil.naive_tally(ent, "c", 55, "A", "C", True)
    assert want == [2, 2, 0, 1, 1, 0, 1, 1]
    np.testing.assert_array_equal(tally(bam, "c", [55], [allele_of("A", "C")], where="host"), [want])
    vcf = tmp_path / "truth.vcf"
    vcf.write_text("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS\nc\t10\t.\tA\tC\t1\tPASS\t.\tGT\t0/1\n")
    with pytest.raises(SystemExit, match="HP:i:12"):
        main(["--tumor_bam_fn", bam, "--truth_vcf_fn", str(vcf), "--output_path", str(tmp_path / "o.txt"), "--where", "host"])
