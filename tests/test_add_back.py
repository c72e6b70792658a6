"""add_back_missing_variants_in_genotyping without a GPU: the library's host path and the module's Python restatement against what the
reference wrote (tests/golden/add_back.json.gz, made by gen_add_back.py), random cases against the naive restatement of tests/addbackutil.py,
the rows the call will not decide, and cto_sort_u64's host path against numpy's stable order."""
import os

import numpy as np
import pytest

import addbackutil as u
import primutil as pu
from conftest import load_json_gz

G = u.golden()
CONFIGS = {c["name"]: c for c in G["configs"]}
SORT_TILE = pu.consts()["SORT_TILE"]          # the library's own, so that the cases below follow the kernels' seams
LINE_TILE = pu.consts()["LINE_TILE"]


def test_the_tile_sizes_are_the_ones_these_cases_were_written_for():
    """a header that changes them moves every seam here with it: look at the cases again, then at these two numbers"""
    assert SORT_TILE == 2048 and LINE_TILE == 16384


def run_config(cf, d, capsys, where="host", restated=False, monkeypatch=None):
    from clairs_to_amd import add_back_missing_variants_in_genotyping as m
    from clairs_to_amd.__main__ import SUBMODULES, dispatch
    assert "add_back_missing_variants_in_genotyping" in SUBMODULES
    u.write_inputs(str(d), G["texts"])
    if restated:
        monkeypatch.setattr(m, "add_back", lambda calls, listed, info, mode, sw, **kw: m.restate(calls, listed, info, mode, sw))
    capsys.readouterr()
    exit_msg = None
    try:
        dispatch("add_back_missing_variants_in_genotyping", u.config_argv(cf, d, where))
    except SystemExit as e:
        exit_msg = str(e.code)
    out_fn = os.path.join(str(d), "out.vcf")
    call_fn = u.config_argv(cf, d)[cf["argv"].index("--call_fn") + 1]
    return dict(stdout=capsys.readouterr().out, exit=exit_msg, output=open(out_fn).read() if os.path.exists(out_fn) else None,
                bak=os.path.exists(call_fn + ".bak"))


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_host_path_writes_the_references_file(tmp_path, capsys, name):
    cf = CONFIGS[name]
    got = run_config(cf, tmp_path / "w", capsys)
    assert got == {k: cf[k] for k in got}


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_python_restatement_writes_the_references_file(tmp_path, capsys, monkeypatch, name):
    cf = CONFIGS[name]
    got = run_config(cf, tmp_path / "w", capsys, restated=True, monkeypatch=monkeypatch)
    assert got == {k: cf[k] for k in got}


def test_fixture_covers_what_it_claims():
    assert len(CONFIGS) >= 20
    sw = CONFIGS["geno_sw"]["output"]
    assert "./.:30:3:5:0:0" in sw and "./.:41:7:2:0:123456789" in sw and "chr1 28 . G T\t.\t.\tG\t." in sw
    assert CONFIGS["both_none"]["exit"].startswith("[ERROR] Both VCF") and CONFIGS["calls_missing"]["bak"] is False


def test_naive_restatement_agrees_with_the_reference_too():
    for name, cf in CONFIGS.items():
        if cf["output"] is None:
            continue
        calls, listed, info, mode, sw = u.config_texts(cf, G["texts"])
        text, counts = u.naive(calls, listed, info, mode, sw)
        assert text.decode() == cf["output"], name
        assert "genotyping: %d, total tumor-only somatic variant calls: %d, added %d variants" % counts in cf["stdout"], name


def test_parser_takes_every_reference_option_and_every_captured_argv():
    from clairs_to_amd.add_back_missing_variants_in_genotyping import build_parser
    mine = {o: a for a in build_parser()._actions for o in a.option_strings}
    assert len(G["parser"]) == 6
    for opt in G["parser"]:
        for o in opt["options"]:
            assert o in mine, o
            assert getattr(mine[o].type, "__name__", None) == opt["type"] and mine[o].default == opt["default"], o
    for cf in CONFIGS.values():
        ns = vars(build_parser().parse_args(cf["argv"]))
        if cf["namespace"] is not None:
            assert {k: ns[k] for k in cf["namespace"]} == cf["namespace"], cf["name"]
    n = 0
    for run in load_json_gz("argv.json.gz")["runs"]:
        for inv in run["invocations"]:
            if inv["submodule"] == "add_back_missing_variants_in_genotyping":
                a = build_parser().parse_args([t.replace("@W@", "/w").replace("@T@", "/t") for t in inv["argv"]])
                assert a.call_fn and a.output_fn and (a.genotyping_mode_vcf_fn or a.hybrid_mode_vcf_fn)
                n += 1
    assert n > 0


@pytest.mark.parametrize("seed,n_list,repeat", [(1, 40, 0), (2, 700, 0), (3, SORT_TILE + 300, 0), (4, 3 * SORT_TILE + 7, 0), (5, 300, SORT_TILE + 50)])
def test_random_cases_against_the_naive_restatement(seed, n_list, repeat):
    from clairs_to_amd.add_back_missing_variants_in_genotyping import add_back, restate
    calls, listed, info = u.random_case(seed, n_list, repeat=repeat)
    for mode in (0, 1):
        for sw in (True, False):
            want = u.naive(calls, listed, info, mode, sw)
            st = {}
            assert add_back(calls, listed, info, mode, sw, where="host", host_threads=1 + seed, stats=st) == want, (mode, sw)
            assert st["restated"] is None and st["host_path"] == 1 and st["n_lines"][1] == n_list + repeat + 2
            assert restate(calls, listed, info, mode, sw) == want, (mode, sw)


HEAD = b"#CHROM\tPOS\n"
UNDECIDED = [
    ("plus", HEAD + b"chr1\t+5\t.\tA\tC\n", b"", "undecided"),
    ("underscore", HEAD + b"chr1\t1_0\t.\tA\tC\n", b"", "undecided"),
    ("pos19", HEAD + b"chr1\t1000000000000000000\t.\tA\tC\n", b"", "undecided"),
    ("pos2to42", HEAD + b"chr1\t4398046511104\t.\tA\tC\n", b"", "undecided"),
    ("count", HEAD + b"chr1\t5\t.\tA\tC\n", b"chr1\t5\tA\t9-A +3\n", "undecided"),
    ("depth", HEAD + b"chr1\t5\t.\tA\tC\n", b"chr1\t5\tA\t 9-A 3\n", "undecided"),
    ("info_pos", HEAD + b"chr1\t5\t.\tA\tC\n", b"chr1\t 5\tA\t9-A 3\n", "undecided"),
    ("crlf", HEAD + b"chr1\t5\t.\tA\tC\r\nchr1\t7\t.\tA\tC\r\n", b"chr1\t5\tA\t9-A 3\n", "non_ascii"),
    ("cr", HEAD + b"chr1\t5\t.\tA\tC\rchr1\t7\t.\tA\tC\n", b"", "non_ascii"),
    ("high", HEAD + b"chr1\t5\t.\tA\tC\t.\t.\tX=\xc3\xa9\n", b"chr1\t5\tA\t9-A 3\n", "non_ascii"),
    ("nbsp", HEAD + b"chr1\xc2\xa05\t.\tA\tC\t.\n", b"", "non_ascii"),
]


@pytest.mark.parametrize("name,listed,info,why", UNDECIDED, ids=[r[0] for r in UNDECIDED])
def test_rows_the_call_does_not_decide_are_counted_and_restated(name, listed, info, why):
    from clairs_to_amd.add_back_missing_variants_in_genotyping import add_back, restate
    calls = HEAD + b"chr1\t7\t.\tA\tG\t9\n"
    for mode in (0, 1):
        st = {}
        got = add_back(calls, listed, info, mode, True, where="host", stats=st)
        assert st["restated"] == why and (st["undecided"] > 0 if why == "undecided" else st["non_ascii"] == 1), st
        assert got == restate(calls, listed, info, mode, True)
    text = restate(calls, listed, info, 0, True)[0]
    if name in ("plus", "underscore", "pos19", "pos2to42"):
        assert text.count(b"./.:0:0:0:0:0") == 1
    if name in ("count", "info_pos"):
        assert b"./.:9:3:0:0:0" in text
    if name == "depth":
        assert b"./.:9:3:0:0:0" in text          # int(' 9') is 9
    if name == "crlf":
        assert text.count(b"\n") == 3 and b"\r" not in text and b"./.:9:3:0:0:0\n" in text and b"chr1\t7\t.\tA\tG\t9\n" in text
    if name == "nbsp":
        assert b"chr1\xc2\xa05\t.\tA\tC\t." in text      # U+00A0 is whitespace to str.split(): CHROM chr1, POS 5


def test_decided_shapes_stay_on_the_fast_path():
    """shapes that look odd but that the rules settle: no digit in a number (int() raises: zeros), empty pieces, leading zeros"""
    from clairs_to_amd.add_back_missing_variants_in_genotyping import add_back
    listed = HEAD + b"chr1\t5\n chr1\t006\t.\tAC\n\tchr1 7 \t\t\n"
    info = b"chr1\t5\tT\tx-A 1\nchr1\t6\tAC\t030-A 007 A\nchr1\t7\t\t4-T 18 - \nshort\t1\t2\n"
    st = {}
    text, counts = add_back(HEAD, listed, info, 0, True, where="host", stats=st)
    assert st["restated"] is None and st["undecided"] == 0 and counts == (3, 0, 3)
    assert text == u.naive(HEAD, listed, info, 0, True)[0]
    assert b"chr1\t5\t.\tT\t.\t.\t.\t.\tGT:DP:AU:CU:GU:TU\t./.:0:0:0:0:0\n" in text and b" chr1\t006\t.\tAC\t." in text and b"./.:30:7:0:0:0" in text


@pytest.mark.parametrize("text,source,line", [(HEAD + b"chr1\t5\n\nchr1\t6\n", 2, 3), (HEAD + b"chr1\t5\n  \t \nchr1\t6\n", 2, 3), (HEAD + b"chr1\n", 2, 2)])
def test_a_line_without_chrom_and_pos_ends_the_run_naming_it(tmp_path, text, source, line):
    from clairs_to_amd.add_back_missing_variants_in_genotyping import BadLine, add_back, main, restate
    for fn in (lambda: add_back(HEAD, text, b"", 0, True, where="host"), lambda: restate(HEAD, text, b"", 0, True),
               lambda: add_back(text, HEAD, b"", 1, True, where="host")):
        with pytest.raises(BadLine) as e:
            fn()
        assert e.value.line == line
    (tmp_path / "list.vcf").write_bytes(text)
    (tmp_path / "calls.vcf").write_bytes(HEAD)
    with pytest.raises(SystemExit) as e:
        main(["--genotyping_mode_vcf_fn", str(tmp_path / "list.vcf"), "--call_fn", str(tmp_path / "calls.vcf"), "--output_fn", str(tmp_path / "o.vcf"),
              "--where", "host"])
    assert "line %d of %s" % (line, tmp_path / "list.vcf") in str(e.value)


SAME = 0x0123456789ABCDEF


def one_odd_key(n, at, byte):
    """every key the same but the one at `at`, which differs in one byte: that pass runs with whole rounds of 64 peers"""
    keys = np.full(n, SAME, dtype=np.uint64)
    keys[at] ^= np.uint64(0x5A << (8 * byte))
    return keys


def sort_cases(rng):
    T = SORT_TILE
    # 16 T: the histogram table (256 cells a tile) no longer fits one trip of the one-workgroup scan; 64 T: the scan takes three launches
    large = (16 * T - 1, 16 * T, 16 * T + 1, 64 * T - 1, 64 * T, 64 * T + 1, 192 * T + 77)
    n_of = (0, 1, 2, 63, 64, 65, 511, 512, 513, T - 1, T, T + 1, 3 * T + 7) + large
    for n in n_of:
        i = np.arange(n, dtype=np.uint64)
        for byte in ((0, 7) if n in large else range(8)):
            for at in sorted(a for a in {0, n - 1, T - 1, T, 511, 512} if 0 <= a < n):          # first, last, at a tile seam, at a wave seam
                yield "one_odd_key byte %d at %d" % (byte, at), n, one_odd_key(n, at, byte)
        for byte in (0, 5):
            yield "ramp64 byte %d" % byte, n, ((i % np.uint64(256)) << np.uint64(8 * byte)) | np.uint64(0x7766004433221100)
            yield "groups_of_8 byte %d" % byte, n, (((i // np.uint64(8)) % np.uint64(256)) << np.uint64(8 * byte)) | np.uint64(0x7766004433221100)
        r = rng.integers(0, 1 << 62, n, dtype=np.uint64)
        yield "equal", n, np.full(n, SAME, dtype=np.uint64)
        yield "random", n, r
        yield "few", n, rng.integers(0, 5, n, dtype=np.uint64) * np.uint64(0x0101010101010101)
        yield "sorted", n, np.sort(r)
        yield "reversed", n, np.sort(r)[::-1].copy()
        yield "top_byte", n, (rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(56)) | np.uint64(0x00ABCDEF01234567)
        yield "bottom_byte", n, rng.integers(0, 256, n, dtype=np.uint64) | np.uint64(0x7766554433221100)
        yield "bit63", n, r | (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63))


def check_sort(where):
    from clairs_to_amd.add_back_missing_variants_in_genotyping import sort_u64
    rng = np.random.default_rng(20261021)
    for name, n, keys in sort_cases(rng):
        pay = rng.permutation(n).astype(np.uint32)
        before = keys.copy()
        k, p = sort_u64(keys, pay, where)
        order = np.argsort(keys, kind="stable")
        assert np.array_equal(keys, before)
        assert np.array_equal(k, keys[order]) and np.array_equal(p, pay[order]), (name, n)
        if name == "equal":
            assert np.array_equal(p, pay)


def test_sort_u64_host_path_is_numpys_stable_order():
    check_sort("host")
