"""select_hetero_snp_for_phasing against the reference's own run (tests/golden/select_hetero.json.gz, made by gen_select_hetero.py in the
build container): the output file and the printed line, byte for byte, for every configuration; and the parser against the reference's
option table and the argv run_clairs_to builds for it.  Host only."""
import gzip
from argparse import Namespace

import pytest

from conftest import load_json_gz
from test_cli_argv import SAMPLE, fill

from clairs_to_amd import select_hetero_snp_for_phasing as sh


@pytest.fixture(scope="module")
def golden():
    return load_json_gz("select_hetero.json.gz")


NAMES = ["chrA_pct0", "chrB_pct0", "chrA_pct01", "chrA_pct05", "chrB_pct05", "chrA_minqual9", "chrA_minqual0", "chrA_pct01_minqual0", "dup_pct0",
         "dup_pct05", "dup_pct03_gz", "absent_contig"]


def test_fixture_holds_the_configurations(golden):
    assert [c["name"] for c in golden["configs"]] == NAMES
    assert sum(c["gz"] for c in golden["configs"]) >= 3
    assert {c["namespace"]["var_pct_full"] for c in golden["configs"]} >= {0.0, 0.1, 0.5}


@pytest.mark.parametrize("name", NAMES)
def test_byte_identical_to_the_reference(golden, name, tmp_path, capsys):
    cf = next(c for c in golden["configs"] if c["name"] == name)
    text = golden["inputs"][cf["vcf"]]
    fn = tmp_path / cf["namespace"]["tumor_vcf_fn"]
    if cf["gz"]:
        with gzip.open(fn, "wt") as f:
            f.write(text)
    else:
        fn.write_text(text)
    ns = dict(cf["namespace"], tumor_vcf_fn=str(fn), output_folder=str(tmp_path / "out" / "vcf"))      # a folder that is not there yet
    capsys.readouterr()
    sh.select_hetero_snp_for_phasing(Namespace(**ns))
    assert capsys.readouterr().out == cf["printed"]
    assert (tmp_path / "out" / "vcf" / (cf["namespace"]["ctg_name"] + ".vcf")).read_text() == cf["output"]


def test_through_the_dispatcher(golden, tmp_path, capsys):
    from clairs_to_amd.__main__ import SUBMODULES, dispatch
    assert "select_hetero_snp_for_phasing" in SUBMODULES
    cf = golden["configs"][0]
    (tmp_path / "in.vcf").write_text(golden["inputs"][cf["vcf"]])
    dispatch("select_hetero_snp_for_phasing", ["--tumor_vcf_fn", str(tmp_path / "in.vcf"), "--output_folder", str(tmp_path / "o"), "--ctg_name", "chrA"])
    assert capsys.readouterr().out == cf["printed"]
    assert (tmp_path / "o" / "chrA.vcf").read_text() == cf["output"]


def test_parser_takes_the_references_options(golden):
    table = golden["parser"]
    assert sorted(o["options"][-1] for o in table) == ["--ctg_name", "--min_qual", "--output_folder", "--tumor_vcf_fn", "--var_pct_full"]
    mine = {a.option_strings[-1]: a for a in sh.build_parser()._actions if a.option_strings}
    for opt in table:
        a = mine[opt["options"][-1]]
        assert (a.nargs, getattr(a.type, "__name__", None), a.default) == (opt["nargs"], opt["type"], opt["default"]), opt
        got = sh.build_parser().parse_args([opt["options"][-1], SAMPLE[opt["type"]]])
        assert getattr(got, a.dest) == a.type(SAMPLE[opt["type"]])
    assert "--min_qual" not in sh.build_parser().format_help()                   # suppressed, as in the reference


def test_every_captured_argv_parses():
    n = 0
    for run in load_json_gz("argv.json.gz")["runs"]:
        for inv in run["invocations"]:
            if inv["submodule"] != "select_hetero_snp_for_phasing":
                continue
            a = sh.build_parser().parse_args(fill(inv["argv"], inv["source"]))
            assert a.ctg_name == "chr20" and a.tumor_vcf_fn.endswith(".vcf") and a.output_folder.startswith("/w/") and a.var_pct_full == 0.0
            n += 1
    assert n >= 1
