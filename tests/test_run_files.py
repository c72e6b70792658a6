"""csrc/run_files.h - the GPU-free file handling of cto_run_chunks - under AddressSanitizer and UBSan: tests/host/run_files_check.cpp
is built once with g++ and run as a child process per case.  Expected values come from the Python mirror (clairs_to_amd.fasta) and
from the interval rules written out below, never from the code under test."""
import gzip
import os
import subprocess

import pytest

from clairs_to_amd.fasta import read_region

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="session")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("run_files") / "run_files_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "clairs_to_amd", "csrc"), os.path.join(ROOT, "tests", "host", "run_files_check.cpp"),
                           "-o", exe, "-lz", "-lpthread"])

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0 and not r.stderr, (args, r.returncode, r.stderr.decode(errors="replace")[-2000:])
        return r.stdout.decode()
    return run


def fnv(data):
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%d %016x\n" % (len(data), h)


def write_fasta(path, contigs, width=7, eol="\n", fai=None):
    """contigs: [(name, bases)] -> FASTA with `width` bases per line + the .fai samtools faidx would write"""
    body, index = b"", []
    for name, seq in contigs:
        body += (">%s%s" % (name, eol)).encode()
        index.append("%s\t%d\t%d\t%d\t%d\n" % (name, len(seq), len(body), width, width + len(eol)))
        for i in range(0, len(seq), width):
            body += (seq[i:i + width] + eol).encode()
    with open(path, "wb") as f:
        f.write(body)
    with open(fai or path + ".fai", "w") as f:
        f.write("".join(index))
    return path


SEQ1 = "ACGTNACGTTGCAAGGCTTAGCATCGATCGGATTACA" * 2 + "GGA"      # 77 bases: 11 lines of 7, no short line
SEQ2 = "TTGACCAGTNNACGGTAGCTAGCATCGA" + "CATG"                  # 32 bases: a final short line of 4
REGIONS = [(1, 7), (7, 8), (3, 30), (1, 77), (70, 77), (-5, 5), (60, 1000), (-5, 1000), (33, 33), (40, 39), (100, 200)]


@pytest.mark.parametrize("eol,lower,alt_fai", [("\n", False, False), ("\r\n", False, False), ("\n", True, False), ("\n", False, True)],
                         ids=["plain", "crlf", "lower_case", "fai_without_extension"])
def test_read_region_equals_the_python_reader(check, tmp_path, eol, lower, alt_fai):
    fa = str(tmp_path / "ref.fa")
    conv = str.lower if lower else str
    write_fasta(fa, [("chr1", conv(SEQ1)), ("chr10", conv(SEQ2))], eol=eol, fai=str(tmp_path / "ref.fai") if alt_fai else None)
    for ctg, seq in (("chr1", SEQ1), ("chr10", SEQ2)):
        for start, end in REGIONS:
            want = read_region(fa, ctg, start, end)
            assert want == seq[max(1, start) - 1:max(0, min(len(seq), end))]          # the mirror itself: clipped, upper case, no line ends
            assert check("region", fa, ctg, start, end) == want + "\n", (ctg, start, end)


def test_read_region_errors(check, tmp_path):
    fa = write_fasta(str(tmp_path / "ref.fa"), [("chr1", SEQ1)])
    assert check("region", fa, "chr2", 1, 5).startswith("error: contig chr2 not in " + fa + ".fai")
    assert check("region", fa, "chr", 1, 5).startswith("error: contig chr not in ")          # a prefix of a name is not the name
    with open(fa + ".fai", "w") as f:
        f.write("chr1\t5000\t6\t7\t8\n")
    assert check("region", fa, "chr1", 1, 5000) == "error: reference index points outside the FASTA file\n"
    gz = str(tmp_path / "packed.fa")
    with open(gz, "wb") as f:
        f.write(gzip.compress(b">chr1\nACGT\n"))
    with open(gz + ".fai", "w") as f:
        f.write("chr1\t4\t6\t4\t5\n")
    assert check("region", gz, "chr1", 1, 4).startswith("error: [ERROR] the reference is gzip / bgzip compressed")
    os.remove(fa + ".fai")
    assert check("region", fa, "chr1", 1, 5) == "error: [ERROR] file %s.fai not found\n" % fa


def merged(rows):
    """sorted; a row that overlaps or touches the one before it extends it"""
    out = []
    for b, e in sorted(rows):
        if out and b <= out[-1][1]:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([b, e])
    return out


BED_ROWS = [("chr1", 500, 600, "x"), ("chr10", 5, 9), ("chr1", 100, 200), ("chr1", 150, 260), ("chr1", 260, 300), ("chr2", 1, 2),
            ("chr1", -20, 10), ("chr1", 301, 310), ("chr1", 120, 130), ("chr1", 900, 950)]


def test_bed_intervals(check, tmp_path):
    bed = str(tmp_path / "c.bed")
    text = "".join("\t".join(str(c) for c in r) + "\n" for r in BED_ROWS[:-1]) + "chr1\t700\n" + "\t".join(str(c) for c in BED_ROWS[-1])
    with open(bed, "w") as f:                    # + a row with two columns (no interval); the last row has no newline
        f.write(text)
    for ctg in ("chr1", "chr10", "chr2", "chr3", "chr"):
        want = merged([max(0, r[1]), r[2]] for r in BED_ROWS if r[0] == ctg)
        assert check("bed", bed, ctg) == "".join("%d %d\n" % (b, e) for b, e in want), ctg
    assert merged([max(0, r[1]), r[2]] for r in BED_ROWS if r[0] == "chr1") == [[0, 10], [100, 300], [301, 310], [500, 600], [900, 950]]
    open(bed, "w").close()
    assert check("bed", bed, "chr1") == ""


INDEL_BED = "# a comment\n\nchr2\t50\t60\nchr1 300 400\n   \nchr1\t10\t10\nchr1\t350\t420\tname\nchr1\t420\t430\nchr10\t7\t7\n#chr1\t1\t2\nchr1\t5\t8"


def test_indel_regions(check, tmp_path):
    rows = {"chr1": [[300, 400], [10, 11], [350, 420], [420, 430], [5, 8]], "chr10": [[7, 8]], "chr2": [[50, 60]]}     # a == b: widened by one
    want = "".join("%s %d %d\n" % (c, b, e) for c in sorted(rows) for b, e in merged(rows[c]))
    plain, named_gz, unnamed_gz = str(tmp_path / "r.bed"), str(tmp_path / "r.bed.gz"), str(tmp_path / "r2.bed")
    with open(plain, "w") as f:
        f.write(INDEL_BED)
    for p in (named_gz, unnamed_gz):
        with open(p, "wb") as f:
            f.write(gzip.compress(INDEL_BED.encode()))
    for p in (plain, named_gz, unnamed_gz):
        assert check("indel_regions", p) == want, p
    with open(plain, "w") as f:
        f.write("chr1\t10\t20\nchr1\t30\t25\n")
    assert check("indel_regions", plain) == "error: [ERROR] Invalid bed input in %s: chr1\t30\t25\n" % plain
    with open(plain, "w") as f:
        f.write("chr1\t10\t20\nchr1\tten\t25\n")
    assert "Invalid bed input in 2-th row" in check("indel_regions", plain)
    assert check("indel_regions", str(tmp_path / "missing.bed")).startswith("error: cannot open")


def test_mapped(check, tmp_path):
    data = bytes(range(256)) * 40 + b"tail"
    plain, packed, empty = str(tmp_path / "d.bin"), str(tmp_path / "d.bin.gz"), str(tmp_path / "empty")
    with open(plain, "wb") as f:
        f.write(data)
    with open(packed, "wb") as f:
        f.write(gzip.compress(data))
    open(empty, "wb").close()
    assert check("map", plain) == fnv(data)
    assert check("map", plain, "sniff") == fnv(data)
    assert check("map", packed) == fnv(data)
    assert check("map", empty) == fnv(b"") and check("map", empty, "sniff") == fnv(b"")
    assert check("map", str(tmp_path / "missing")).startswith("error: cannot open")
    assert check("map", str(tmp_path / "missing.gz")).startswith("error: cannot open")


def test_capture_stdout(check):
    want = b"".join(b"%063d\n" % i for i in range(4200))                 # 268 800 bytes: several pipe buffers
    assert len(want) >= 256 * 1024
    assert check("spawn", "/bin/sh", "-c", 'i=0; while [ $i -lt 4200 ]; do printf "%063d\\n" $i; i=$((i+1)); done') == fnv(want)
    assert check("spawn", "/bin/sh", "-c", "printf abc") == fnv(b"abc")
    assert "mpileup failed (exit status 3)" in check("spawn", "/bin/sh", "-c", "printf abc; exit 3")
    assert check("spawn", "/no/such/program", "x").startswith("error: cannot run /no/such/program")
