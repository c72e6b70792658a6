"""nonsomatic_tagging's host side against what the reference wrote (tests/golden/nonsomatic.json.gz, made by gen_nonsomatic.py): the parser,
the header, the rows from a given hit set, the aggregate TSV and its summary, the reference's parse of the lines the device hands back.
No GPU needed: the device scan is tests/test_gpu_nonsomatic.py."""
import base64
import io
import os
from contextlib import redirect_stdout

import pytest

from conftest import load_json_gz

SAMPLE = {"int": "7", "float": "0.25", "str": "x", "str2bool": "True", "str_none": "None", None: "x"}


@pytest.fixture(scope="module")
def golden():
    return load_json_gz("nonsomatic.json.gz")


def parser():
    from clairs_to_amd import nonsomatic_tagging
    return nonsomatic_tagging.build_parser()


def test_every_reference_option_is_accepted(golden):
    table = golden["parser"]
    assert len(table) >= 15
    argv = []
    for opt in table:
        name = opt["options"][-1]
        a = [name] if opt["action"] == "_StoreTrueAction" else [name, SAMPLE[opt["type"]]]
        parser().parse_args(a)
        argv += a
    parser().parse_args(argv)


def test_the_argv_run_clairs_to_builds_parses():
    from test_cli_argv import fill
    runs = load_json_gz("argv.json.gz")["runs"]
    n = 0
    for run in runs:
        for inv in run["invocations"]:
            if inv["submodule"] != "nonsomatic_tagging":
                continue
            argv = [t for t in fill(inv["argv"], inv["source"]) if t != "--do_not_print_nonsomatic_calls"]
            a = parser().parse_args(argv)
            assert a.print_sample_nonsomatic_summary_from_tsv or a.pileup_vcf_fn
            n += 1
    assert n >= 4


def test_the_flag_the_reference_parser_lacks_exits_2():
    with pytest.raises(SystemExit) as e:
        parser().parse_args(["--pileup_vcf_fn", "x.vcf", "--do_not_print_nonsomatic_calls"])
    assert e.value.code == 2


def materialise(tmp_path, files):
    for rel, b64 in files.items():
        p = tmp_path / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(base64.b64decode(b64))


def hits_from_output(text, n_pon):
    """the hit set of every PoN as the reference's output shows it: the PoN_i flags of the NonSomatic rows"""
    hits = [set() for _ in range(n_pon)]
    for row in text.split("\n"):
        if not row or row.startswith("#"):
            continue
        c = row.split("\t")
        if c[6] == "NonSomatic":
            for flag in c[7].split(";"):
                if flag.startswith("PoN_"):
                    hits[int(flag[4:]) - 1].add((c[0], int(c[1])))
    return hits


@pytest.mark.parametrize("name", ["ctg_four_kinds", "all_contigs", "options", "aggregate"])
def test_header_and_rows_from_the_reference_hit_sets(golden, name, tmp_path):
    from clairs_to_amd import nonsomatic_tagging as nt
    sc = next(s for s in golden["scenarios"] if s["name"] == name)
    materialise(tmp_path, sc["inputs"])
    for run in sc["runs"]:
        a = parser().parse_args(run["argv"])
        if a.print_sample_nonsomatic_summary_from_tsv or a.disable_print_nonsomatic_calls:
            continue
        want = base64.b64decode(sc["outputs"][a.output_vcf_fn]).decode()
        header, calls = nt.read_pileup_vcf(str(tmp_path / a.pileup_vcf_fn), a.ctg_name, a.show_ref, a.input_filter_tag)
        sets = nt.call_sets(calls, a.ctg_name, a.show_ref)
        pons = a.panel_of_normals.split(",") if a.panel_of_normals else []
        hits = hits_from_output(want, len(pons))
        if a.ctg_name is not None:
            hits = [{(a.ctg_name, p) for _, p in h} for h in hits]
        info = "".join(line + "\n" for line in want.split("\n") if line.startswith("##INFO=<ID=PoN_"))
        new_header = nt.with_info_lines(header, info) if info else header
        out = tmp_path / ("mine_" + os.path.basename(a.output_vcf_fn))
        nt.write_output(str(out), new_header, sets, hits, a.disable_print_nonsomatic_calls)
        assert out.read_text() == want, run["argv"]


def test_aggregate_tsv_and_sample_summary(golden, tmp_path):
    from clairs_to_amd import nonsomatic_tagging as nt
    sc = next(s for s in golden["scenarios"] if s["name"] == "aggregate")
    want_tsv = base64.b64decode(sc["outputs"]["vcf_output/summary.tsv"]).decode()
    tsv = tmp_path / "vcf_output" / "summary.tsv"
    rows = [ln.split("\t") for ln in want_tsv.split("\n") if ln and not ln.startswith("#")]
    pons = want_tsv.split("\n")[0].split("\t")[1:]
    for r in rows:
        nt.append_summary_row(str(tsv), r[0], [int(x) for x in r[1:]], pons)
    assert tsv.read_text() == want_tsv
    buf = io.StringIO()
    with redirect_stdout(buf):
        nt.print_sample_summary(str(tsv))
    assert buf.getvalue() == sc["runs"][-1]["stdout"]


def test_host_reparse_follows_python_int_and_strip():
    from clairs_to_amd import nonsomatic_tagging as nt
    sets = {"chr1": {123: dict(ref="A", alt="G"), 77: dict(ref="C", alt="T")}}
    lines = [(1, b"chr1\t000123\t.\tA\tC,G\n"), (2, b"chr1\t+77\t.\tC\tT\r\n"), (3, b"chr1\t7_7\t.\tC\tT\n"), (4, b"\xc2\xa0chr1\t77\t.\tC\tT\n"),
             (5, b"chr2\tbad\t.\tA\tG\n")]
    hits = set()
    nt.apply_host_lines(lines[:4], sets, None, True, hits, "p.vcf")
    assert hits == {("chr1", 123), ("chr1", 77)}
    nt.apply_host_lines(lines[4:], sets, None, True, hits, "p.vcf")          # not a contig of the calls: skipped before int()
    with pytest.raises(nt.PonError, match="p.vcf: line 5"):
        nt.apply_host_lines(lines[4:], sets, "chr1", True, set(), "p.vcf")    # --ctg_name: int() sees every line
    h = set()
    nt.apply_host_lines([(1, b"chr1\t123\t.\tT\tC\n")], sets, "chr1", False, h, "p.vcf")
    assert h == {("chr1", 123)}


def test_tbi_reader_against_an_index_built_by_hand(tmp_path):
    """cto_tbi_contig_chunks (the chunks cto_pon_match_file reads for one contig) on the .tbi tests/ponutil.py assembles field by field: the
    chunks, mapped through the BGZF block table to the inflated text, hold exactly that contig's records; a contig the index does not name
    has none; bytes that are no index are refused"""
    import random
    import numpy as np
    from clairs_to_amd import _lib
    from ponutil import bgzf_compress, tbi_bytes, BGZF_EOF
    rng = random.Random(3)
    lines = ["##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\n"]
    for ctg in ("chr1", "chr2", "chrX"):
        pos = 1
        for _ in range(3000):
            pos += rng.randint(1, 120)                       # spans several 16 kb windows and bins of more than one level
            lines.append("%s\t%d\t.\t%s\tG\n" % (ctg, pos, "A" * rng.choice((1, 1, 3))))
    text = "".join(lines).encode()
    comp, blocks = bgzf_compress(text, block=3000)
    tbi = tbi_bytes(text, blocks, len(comp) - len(BGZF_EOF))
    start = {coff: ustart for coff, ustart, _ in blocks}
    start[len(comp) - len(BGZF_EOF)] = len(text)

    def chunks(ctg, blob=tbi):
        out = np.zeros(2 * 4096, np.uint64)
        n = _lib.lib.cto_tbi_contig_chunks(blob, len(blob), ctg.encode(), out.ctypes.data, 4096)
        return n, [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(max(n, 0))]

    for ctg in ("chr1", "chr2", "chrX"):
        n, cs = chunks(ctg)
        assert n >= 1
        got = b"".join(text[start[b >> 16] + (b & 0xffff):start[e >> 16] + (e & 0xffff)] for b, e in cs)
        want = b"".join(ln.encode() for ln in lines if ln.startswith(ctg + "\t"))
        assert got == want, ctg
    assert chunks("chr7") == (0, [])
    assert chunks("chr1", blob=b"\x1f\x8b" + b"\0" * 40)[0] < 0
