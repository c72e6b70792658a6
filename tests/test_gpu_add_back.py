"""add_back_missing_variants_in_genotyping on the device: the kernels' bytes against the host path's on the reference's fixture and on random
cases, cto_sort_u64 against numpy's stable order, the command at the kernels' own edges, and the chain extract_candidates_calling ->
add_back on real _hybrid_info files."""
import os

import pytest

import addbackutil as u
from test_add_back import CONFIGS, G, HEAD, LINE_TILE, SORT_TILE, check_sort, run_config
from test_gpu_cli_argv import Work, golden  # noqa: F401  (fixture)
from test_gpu_region_modes import _opt

pytestmark = pytest.mark.gpu


def both(calls, listed, info, mode, sw, naive=True):
    """the device's (bytes, counts), after holding them to the host path's and, on request, to the naive restatement's"""
    from clairs_to_amd.add_back_missing_variants_in_genotyping import add_back
    sd, sh = {}, {}
    dev = add_back(calls, listed, info, mode, sw, where="device", stats=sd)
    host = add_back(calls, listed, info, mode, sw, where="host", stats=sh)
    assert sd["restated"] is None and sh["restated"] is None and sd["host_path"] == 0 and sh["host_path"] == 1
    assert sd["n_lines"] == sh["n_lines"] and sd["n_rows"] == sh["n_rows"]
    assert dev[1] == host[1]
    assert dev[0] == host[0]
    if naive:
        assert dev == u.naive(calls, listed, info, mode, sw)
    return dev


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_device_writes_the_references_file(tmp_path, capsys, name):
    cf = CONFIGS[name]
    got = run_config(cf, tmp_path / "w", capsys, where="device")
    assert got == {k: cf[k] for k in got}
    if cf["output"] is not None:
        calls, listed, info, mode, sw = u.config_texts(cf, G["texts"])
        assert both(calls, listed, info, mode, sw)[0].decode() == cf["output"]


@pytest.mark.parametrize("seed,n_list,repeat", [(1, 40, 0), (2, 700, 0), (3, SORT_TILE + 300, 0), (4, 3 * SORT_TILE + 7, 0), (5, 300, SORT_TILE + 50),
                                                (6, 16 * SORT_TILE + 300, 0), (7, 64 * SORT_TILE + 300, 0)])
def test_random_cases_device_against_host(seed, n_list, repeat):
    """The last two lists sort more than 16 and more than 64 tiles of records: the sort's histogram table takes a second trip of the
    one-workgroup scan, then the scan's three launches.  At 64 tiles the naive restatement takes 1.4 s a run on the CPU, 5.8 s for the
    four: there it checks one of the four, the host path all of them."""
    calls, listed, info = u.random_case(seed, n_list, repeat=repeat)
    for mode in (0, 1):
        for sw in (True, False):
            both(calls, listed, info, mode, sw, naive=n_list < 64 * SORT_TILE or (mode == 1 and sw))


def test_sort_u64_device_is_numpys_stable_order():
    check_sort("device")


def test_undecided_rows_are_reported_by_the_device_too():
    from clairs_to_amd.add_back_missing_variants_in_genotyping import add_back, restate
    calls = HEAD + b"chr1\t7\t.\tA\tG\t9\n"
    for listed, info, why in ((HEAD + b"chr1\t+5\t.\tA\tC\n", b"", "undecided"), (HEAD + b"chr1\t5\t.\tA\tC\n", b"chr1\t5\tA\t9-A 1_0\n", "undecided"),
                              (HEAD + b"chr1\t5\t.\tA\tC\r\n", b"", "non_ascii"), (HEAD + b"chr1\t5\t.\t\xc3\xa9\tC\n", b"", "non_ascii")):
        st = {}
        assert add_back(calls, listed, info, 0, True, where="device", stats=st) == restate(calls, listed, info, 0, True)
        assert st["restated"] == why and st["host_path"] == 0


def test_no_records_one_row_and_header_only():
    assert both(b"", b"", b"", 0, True) == (b"", (0, 0, 0))
    assert both(b"", b"", b"", 1, False) == (b"", (0, 0, 0))
    assert both(HEAD, HEAD, b"", 1, True) == (HEAD, (0, 0, 0))
    assert both(HEAD + b"##more\n", b"", b"chr1\t5\tA\t3-A 3\n", 0, True) == (HEAD + b"##more\n", (0, 0, 0))
    one = both(b"", b"chr1\t5", b"chr1\t5\tA\t3-A 3", 0, True)
    assert one == (b"chr1\t5\t.\tA\t.\t.\t.\t.\tGT:DP:AU:CU:GU:TU\t./.:3:3:0:0:0\n", (1, 0, 1))
    assert both(b"chr1\t5\t.\tA\tC", b"chr1\t5", b"", 1, True) == (b"chr1\t5\t.\tA\tC", (1, 1, 0))


def sized(size, row_at=None):
    """a calls text of exactly `size` bytes whose last line, a lone '#', starts at its last byte; row_at: a record line starts there"""
    rows = [HEAD]
    n, p = len(HEAD), 10
    target = (row_at if row_at is not None else size - 1)
    while True:
        row = b"chr1\t%d\t.\tA\tC\t5\tPASS\tX=\n" % p
        if n + len(row) + 40 > target:
            break
        rows.append(row)
        n += len(row)
        p += 3
    last = b"chr1\t%d\t.\tA\tC\t5\tPASS\tX=" % p
    rows.append(last + b"x" * (target - n - len(last) - 1) + b"\n")
    text = b"".join(rows)
    assert len(text) == target
    if row_at is not None:
        tail = b"chr2\t77\t.\tG\tT\t1\tPASS\tY="
        text += tail + b"y" * (size - 2 - len(text) - len(tail)) + b"\n"
    text += b"#"
    assert len(text) == size and text[size - 1:] == b"#" and text[size - 2:size - 1] == b"\n"
    return text


@pytest.mark.parametrize("size,row_at", [(LINE_TILE - 1, None), (LINE_TILE, None), (LINE_TILE + 1, None), (2 * LINE_TILE + 33, LINE_TILE),
                                         (2 * LINE_TILE + 1, 2 * LINE_TILE - 40)])
def test_text_around_the_line_tile(size, row_at):
    calls = sized(size, row_at)
    listed = HEAD + b"chr1\t13\t.\tA\tC\nchr2\t77\nchr1\t11\t.\tA\tC\n"
    text, counts = both(calls, listed, b"chr1\t11\tA\t4-A 4\n", 1, True)
    assert text.startswith(HEAD + b"#chr1\t10\t") and counts[0] == 3 and counts[2] == (1 if row_at is not None else 2)
    if row_at is not None:
        assert calls[row_at:row_at + 8] == b"chr2\t77\t" and text.count(b"chr2\t77\t.\tG\tT") == 1
    # the same text as the list and as the info: their line starts go through the same passes
    both(HEAD, calls, b"", 0, True)
    both(HEAD, HEAD + b"chr1\t10\nchr1\t11\n", calls, 0, True)


def test_one_key_repeated_beyond_a_sort_tile():
    n = SORT_TILE + 77
    calls = HEAD + b"".join(b"chr1\t500\t.\tA\tC\t%d\n" % k for k in range(n)) + b"chr1\t400\t.\tA\tC\tx\n"
    listed = HEAD + b"".join(b"chr1\t600\t.\tA\tC\t%d\n" % k for k in range(n)) + b"chr1\t500\t.\tA\tC\tl\n"
    info = b"".join(b"chr1\t600\tG\t%d-A %d\n" % (k, k) for k in range(n))
    text, counts = both(calls, listed, info, 1, True)
    assert counts == (2, 2, 1)
    assert text == HEAD + b"chr1\t400\t.\tA\tC\tx\n" + b"chr1\t500\t.\tA\tC\t%d\n" % (n - 1) + (
        b"chr1\t600\t.\tG\t.\t.\t.\t.\tGT:DP:AU:CU:GU:TU\t./.:%d:%d:0:0:0\n" % (n - 1, n - 1))


def test_large_positions_and_many_contigs():
    pos = (1, 2147483647, 2147483648, 4294967295, 4294967296, (1 << 42) - 1)
    ctgs = ["ctg%02d" % k for k in range(53)] + ["chrY", "22", "chr3", "Y", "chr10", "1", "chrX"]          # 60 contigs
    listed = HEAD + "".join("%s\t%d\t.\tA\tC\n" % (c, p) for c in ctgs for p in reversed(pos)).encode()
    calls = HEAD + "".join("%s\t%d\t.\tA\tC\tcalled\n" % (c, 2147483647) for c in ctgs[::2]).encode()
    info = "".join("%s\t%d\tC\t%d-T %d\n" % (c, p, p, p) for c in ctgs for p in pos).encode()
    text, counts = both(calls, listed, info, 0, True)
    assert counts == (360, 30, 330)
    rows = [ln.split(b"\t") for ln in text.split(b"\n")[1:-1]]
    order = [r[0].decode() for r in rows[::6]]
    assert order[:7] == ["chr3", "chr10", "chrX", "chrY", "1", "22", "Y"]
    assert order[7:] == [c for c in ctgs[::2] if c.startswith("ctg")] + [c for c in ctgs[1::2] if c.startswith("ctg")]      # first seen in the calls, then in the list
    assert all([int(r[1]) for r in rows[k:k + 6]] == list(pos) for k in range(0, 360, 6))
    assert b"ctg01\t4398046511103\t.\tC\t.\t.\t.\t.\tGT:DP:AU:CU:GU:TU\t./.:4398046511103:0:0:0:4398046511103\n" in text


def test_long_row_next_to_a_short_one_and_counts_of_1_and_18_digits():
    big = b"Z" * 5000
    calls = HEAD + b"chr1\t5\t.\n" + b"chr1\t6\t.\tA\tC\t1\tPASS\t" + big + b"\tGT\t0/1\nchr1\t7\t.\n"
    listed = HEAD + b"chr1\t6\nchr1\t8\t.\tA\tC\t1\tPASS\t" + big + b"\tGT\t0/1\t" + big + b"\nchr1\t9\t.\n"
    info = b"chr1\t8\t" + big + b"\t0-A 9 C 999999999999999999 G 0 T 100000000000000000\nchr1\t9\tA\t999999999999999999-A 1\n"
    assert len(b"chr1\t5\t.\n") == 9
    text, counts = both(calls, listed, info, 1, True)
    assert counts == (3, 3, 2)
    assert b"chr1\t8\t.\t" + big + b"\t.\t.\t.\t.\tGT:DP:AU:CU:GU:TU\t./.:0:9:999999999999999999:0:100000000000000000\t" + big + b"\n" in text
    assert text.endswith(b"chr1\t9\t.\tA\t.\t.\t.\t.\tGT:DP:AU:CU:GU:TU\t./.:999999999999999999:1:0:0:0\n")


def test_a_list_in_which_every_row_is_called():
    calls, listed, info = u.random_case(11, 500, call_share=1.0)
    for mode in (0, 1):
        text, counts = both(calls, listed, info, mode, True)
        assert counts[2] == 0 and b"./." not in text


def test_chain_from_extract_candidates_calling(tmp_path, golden, capsys):  # noqa: F811
    """genotyping mode: extract_candidates_calling writes the _hybrid_info files, add_back reads them"""
    from clairs_to_amd.add_back_missing_variants_in_genotyping import main
    rec = golden["executed"]["ont_genotyping"]
    with Work(tmp_path, "ont_genotyping", rec, golden) as wk:
        for sub, argv in rec["step1_argv"]:
            wk.run(sub, argv)
        cand = os.path.join(wk.w, wk.tmp, "candidates")
        list_fn = wk.real(_opt(rec["step1_argv"][0][1], "--genotyping_mode_vcf_fn"))
    files = sorted(f for f in os.listdir(cand) if f.endswith("_hybrid_info"))
    assert len(files) == 3
    infos = u.naive_info(b"".join(open(os.path.join(cand, f), "rb").read() for f in files))
    list_rows = [ln for ln in open(list_fn).read().split("\n") if ln and ln[0] != "#"]
    keys = [(ln.split("\t")[0], int(ln.split("\t")[1])) for ln in list_rows]
    assert len(keys) == len(set(keys)) >= 3 and any(k in infos for k in keys)
    called = {k: "%s\t%d\t.\tA\tC\t17.5\tPASS\tH\tGT:GQ:DP:AF\t0/1:17:40:0.3\n" % k for k in keys[::3]}
    head = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n"
    (tmp_path / "calls.vcf").write_text(head + "".join(called.values()))
    capsys.readouterr()
    main(["--genotyping_mode_vcf_fn", list_fn, "--call_fn", str(tmp_path / "calls.vcf"), "--output_fn", str(tmp_path / "out.vcf"), "--candidates_folder", cand,
          "--where", "device"])
    assert "genotyping: %d, total tumor-only somatic variant calls: %d, added %d variants" % (len(keys), len(called), len(keys) - len(called)) in capsys.readouterr().out
    out = open(tmp_path / "out.vcf").read()
    assert out.startswith(head)
    rows = [ln + "\n" for ln in out[len(head):].split("\n") if ln]
    assert [(r.split("\t")[0], int(r.split("\t")[1])) for r in rows] == sorted(keys, key=lambda k: (u.MAJOR.index(k[0]), k[1]))      # every position once, in order
    n_info = 0
    for r in rows:
        c = r.rstrip("\n").split("\t")
        k = (c[0], int(c[1]))
        if k in called:
            assert r == called[k]
            continue
        want = u.naive_counts(infos[k][1]) if k in infos else [0] * 5
        assert c[4:9] == [".", ".", ".", ".", "GT:DP:AU:CU:GU:TU"] and c[9] == "./.:" + ":".join(str(v) for v in want), r
        n_info += k in infos and want[0] > 0
    assert n_info >= 1
