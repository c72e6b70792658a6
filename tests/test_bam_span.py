"""csrc/bam_span.h - the GPU-free tables of the BAM front end the device consumers share - under AddressSanitizer and UBSan:
tests/host/bam_span_check.cpp is built once with g++ and run as a child process per case.  Expected values come from the rules written
out below, never from the code under test."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="session")
def check(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_span")
    exe = str(d / "bam_span_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "clairs_to_amd", "csrc"), os.path.join(ROOT, "tests", "host", "bam_span_check.cpp"),
                           "-o", exe])

    def run(blocks, voffs, sizes):
        fn = str(d / "case.txt")
        with open(fn, "w") as f:
            f.write("%d\n" % len(blocks) + "".join("%d %d\n" % b for b in blocks))
            f.write("%d\n" % len(voffs) + "".join("%d\n" % v for v in voffs))
            f.write("%d\n" % len(sizes) + "".join("%d\n" % s for s in sizes))
        r = subprocess.run([exe, fn], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr.decode(errors="replace")[-2000:])
        out = {}
        for line in r.stdout.decode().splitlines():
            key, *vals = line.split()
            out[key] = [int(v) for v in vals]
        return out
    return run


def voff(coff, uoff):
    return (coff << 16) | uoff


def span_tables(blocks, voffs):
    """blocks: (file offset, inflated size), ascending.  The inflated blocks end to end make the linear stream; a virtual offset
    (coff << 16 | uoff) names a byte of it when coff is the file offset of a block of the table and uoff <= that block's size
    (== size: the next block's first byte)"""
    lin_off = [0]
    for _, isize in blocks:
        lin_off.append(lin_off[-1] + isize)
    at = {off: k for k, (off, _) in enumerate(blocks)}
    kept = set()
    for v in voffs:
        coff, uoff = v >> 16, v & 0xffff
        if coff in at and uoff <= blocks[at[coff]][1]:
            kept.add(lin_off[at[coff]] + uoff)
    return lin_off, sorted(kept) + [lin_off[-1]], len(kept)


def upload_parts(sizes):
    """every part 256-byte aligned, rounded up to 256 bytes, with 256 bytes behind it"""
    offs, total = [], 0
    for s in sizes:
        offs.append(total)
        total += -(-s // 256) * 256 + 256
    return offs, total


B3 = [(1000, 500), (1300, 65536), (9000, 77)]
CASES = {
    "one_block_one_offset": ([(0, 100)], [voff(0, 36)]),
    "uoff_equal_isize_is_kept": (B3, [voff(1000, 500), voff(1300, 0)]),                  # the same byte twice, by two names
    "uoff_past_isize_dropped": (B3, [voff(1000, 501), voff(9000, 78), voff(1300, 7)]),
    "coff_between_blocks_dropped": (B3, [voff(1001, 0), voff(1299, 3), voff(8999, 0), voff(9000, 5)]),
    "coff_before_first_and_after_last_dropped": (B3, [voff(0, 0), voff(999, 10), voff(9001, 0), voff(1 << 40, 0), voff(1000, 1)]),
    "duplicates_and_descending_order": (B3, [voff(9000, 76), voff(9000, 76), voff(1300, 65535), voff(1300, 40), voff(1000, 499), voff(1000, 499),
                                            voff(1000, 0)]),
    "empty_block_in_the_middle": ([(10, 300), (200, 0), (228, 400)], [voff(200, 0), voff(228, 0), voff(10, 300), voff(228, 399), voff(200, 1)]),
    "every_offset_dropped": (B3, [voff(5, 0), voff(1000, 9999), voff(9000, 78)]),
    "no_offsets_at_all": (B3, []),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_span_tables(check, name):
    blocks, voffs = CASES[name]
    lin_off, starts, n_chains = span_tables(blocks, voffs)
    got = check(blocks, voffs, [])
    assert got["lin_off"] == lin_off and got["len"] == [lin_off[-1]]
    assert got["starts"] == starts and got["n_chains"] == [n_chains]


def test_span_tables_cases_are_what_they_say():
    """the expected values of the named edge cases, spelled out (so that a slip in span_tables above cannot hide one in the code)"""
    assert span_tables(*CASES["one_block_one_offset"]) == ([0, 100], [36, 100], 1)
    assert span_tables(*CASES["uoff_equal_isize_is_kept"])[1:] == ([500, 66113], 1)
    assert span_tables(*CASES["uoff_past_isize_dropped"])[1:] == ([507, 66113], 1)
    assert span_tables(*CASES["coff_between_blocks_dropped"])[1:] == ([66041, 66113], 1)
    assert span_tables(*CASES["coff_before_first_and_after_last_dropped"])[1:] == ([1, 66113], 1)
    assert span_tables(*CASES["duplicates_and_descending_order"])[1:] == ([0, 499, 540, 66035, 66112, 66113], 5)
    assert span_tables(*CASES["empty_block_in_the_middle"]) == ([0, 300, 300, 700], [300, 699, 700], 2)
    assert span_tables(*CASES["every_offset_dropped"])[1:] == ([66113], 0)


@pytest.mark.parametrize("sizes", [[0], [256], [257], [80, 0, 256, 257, 1, 255, 4096, 3], [0, 0]], ids=lambda s: "_".join(map(str, s)))
def test_upload_parts(check, sizes):
    offs, total = upload_parts(sizes)
    got = check([(0, 1)], [], sizes)
    assert got["offsets"] == offs and got["total"] == [total]
    assert got["staged"] == [sum(sizes)]
    assert all(o % 256 == 0 for o in offs) and all(b - a >= s + 256 for a, b, s in zip(offs, offs[1:] + [total], sizes))


def test_upload_parts_spelled_out():
    assert upload_parts([0, 256, 257, 1]) == ([0, 256, 768, 1536], 2048)
