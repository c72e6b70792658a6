"""csrc/bam_host.h - the host's one reader of BGZF, the binning indices and BAM alignment records - under AddressSanitizer and UBSan:
tests/host/bam_host_check.cpp is built once with g++ and run as a child process per case, once with libdeflate (where the machine has
it) and once with zlib.  Expected rows come from the read lists the test wrote and bamutil.effective_cigar, never from the library."""
import os
import struct
import subprocess

import numpy as np
import pytest

import bamrecutil
from bamutil import _bgzf_block, _record, effective_cigar, ref_len_of, write_bam
from bamrecutil import _cg, _read, _tag, query_len_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="session")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("bam_host") / "bam_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "clairs_to_amd", "csrc"), os.path.join(ROOT, "tests", "host", "bam_host_check.cpp"),
                           "-o", path, "-lz", "-ldl"])
    return path


@pytest.fixture(params=["libdeflate", "zlib"])
def check(exe, request):
    env = dict(os.environ)
    env.pop("CTO_NO_LIBDEFLATE", None)
    if request.param == "zlib":
        env["CTO_NO_LIBDEFLATE"] = "1"

    def run(*args):
        """-> (exit status, stdout lines); the sanitizers have nothing to say"""
        r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert not r.stderr and r.returncode in (0, 1), (r.returncode, r.stderr.decode(errors="replace")[-2000:])
        return r.returncode, r.stdout.decode().splitlines()
    return run


def cigar_text(cigar):
    return "".join("%d%s" % (n, op) for op, n in cigar) or "*"


def rows(reads, ref_index, start, end):
    """what the reader yields for start-end (1-based, inclusive) of the contig: every record that begins at or before `end` and is
    not wholly in front of `start` (a record without a reference base counts as one base long), with the CIGAR a reader has to use;
    enters = its operations add up to l_seq, it has a reference base and reaches `start`; then the values of its HP fields (`hp`)"""
    out = []
    for r in reads:
        eff = effective_cigar(r)
        rl, ql = ref_len_of(eff), query_len_of(eff)
        if r["ref"] != ref_index or r["pos"] >= end or r["pos"] + max(rl, 1) <= start - 1:
            continue
        enters = ql == len(r["seq"]) and rl > 0 and r["pos"] + rl > start - 1
        out.append(" ".join(map(str, [r["pos"], r["flag"], r["mapq"], len(r["seq"]), cigar_text(eff), rl, ql, int(enters)] + r.get("hp", []))))
    return out


# ------------------------------------------------------------------------------------------------ auxiliary fields
# the layouts the issue of a shared walker names; the whole-contig case below walks all 49
NAMED_LAYOUTS = ["b_S_7", "xi_bi_before", "cg_overrun", "z_to_record_end", "z_no_nul", "unknown_type", "b_header_cut", "cg_wrong_qlen"]


def test_aux_layouts_all(check):
    c = bamrecutil.aux_case()
    want = rows(c["reads"], 0, 1, c["length"])
    assert len(want) == len(c["reads"]) == 2 * len(c["layouts"]) and len(c["layouts"]) == 49
    assert check(c["bam"], bamrecutil.AUX_CTG, 1, c["length"]) == (0, want)


@pytest.mark.parametrize("name", NAMED_LAYOUTS)
def test_aux_layout(check, name):
    c = bamrecutil.aux_case()
    read, taken = next((r, t) for n, r, t in c["layouts"] if n == name)
    start, end = bamrecutil.aux_region(read)
    want = rows(c["reads"], 0, start, end)
    mine = next(w for w in want if w.startswith("%d " % read["pos"]))
    # spelled out: the CG tag's operations when it is taken, else the placeholder <l_seq>S<n>N
    assert mine.split()[4] == (cigar_text(read["cigar"]) if taken else "%dS%dN" % (len(read["seq"]), ref_len_of(read["cigar"])))
    assert mine.split()[7] == str(int(name != "cg_wrong_qlen"))
    assert check(c["bam"], bamrecutil.AUX_CTG, start, end) == (0, want)


HP_VALUES = {"c": ("<b", -3), "C": ("<B", 200), "s": ("<h", -300), "S": ("<H", 60000), "i": ("<i", -70000), "I": ("<I", 4000000000)}


def test_hp_of_every_integer_type(check, tmp_path):
    rng = np.random.default_rng(7)
    nm = _tag("NM", "i", struct.pack("<i", 3))
    reads = []
    for k, (ty, (fmt, v)) in enumerate(HP_VALUES.items()):
        reads.append(_read(rng, "hp_%s" % ty, 0, 100 + 30 * k, [("M", 25)], aux=nm + _tag("HP", ty, struct.pack(fmt, v)) + nm, hp=[v]))
    # no integer: not printed; an integer cut short by the record's end: not read; behind an unknown type: not reached; two of them: both
    reads.append(_read(rng, "hp_z", 0, 400, [("M", 25)], aux=_tag("HP", "Z", b"1\0"), hp=[]))
    reads.append(_read(rng, "hp_f", 0, 410, [("M", 25)], aux=_tag("HP", "f", struct.pack("<f", 2.0)), hp=[]))
    reads.append(_read(rng, "hp_cut", 0, 420, [("M", 25)], aux=nm + _tag("HP", "i", b"\2\0"), hp=[]))
    reads.append(_read(rng, "hp_s_cut", 0, 425, [("M", 25)], aux=nm + _tag("HP", "s", b"\2"), hp=[]))
    reads.append(_read(rng, "hp_behind_unknown", 0, 430, [("M", 25)], aux=_tag("XQ", "?", b"\1") + _tag("HP", "C", b"\2"), hp=[]))
    reads.append(_read(rng, "hp_twice", 0, 440, [("M", 25)], aux=_tag("HP", "C", b"\1") + _cg([("M", 25)]) + _tag("HP", "c", b"\xff"), hp=[1, -1]))
    bam = str(tmp_path / "hp.bam")
    write_bam(bam, [("hp", 2000)], reads)
    want = rows(reads, 0, 1, 2000)
    assert [w.split()[8:] for w in want[:6]] == [["-3"], ["200"], ["-300"], ["60000"], ["-70000"], ["4000000000"]]
    assert check(bam, "hp", 1, 2000) == (0, want)


# ------------------------------------------------------------------------------------------------ BGZF
def _small_reads(n, ref=0):
    rng = np.random.default_rng(n)
    return [_read(rng, "r%02d" % i, ref, 50 + 20 * i, [("M", 20), ("I", 2), ("M", 18), ("D", 3), ("M", 10)], flag=16 * (i & 1)) for i in range(n)]


def test_record_ends_at_block_end_and_record_straddles(check, tmp_path):
    reads = _small_reads(6)
    header = 12 + 4 + len("blk") + 1 + 4
    n = len(_record(reads[0], 0))
    bam = str(tmp_path / "blocks.bam")
    # block 0: the header and read 0, to its last byte; block 1: half of read 1; block 2: the rest of it and what follows
    info = write_bam(bam, [("blk", 1000)], reads, block_payload=[header + n, n // 2, 60000])
    assert info["block_sizes"][:2] == [header + n, n // 2] and len(info["block_sizes"]) == 3
    assert info["record_spans"][0][1] == header + n and info["record_spans"][1][0] == header + n < header + n + n // 2 < info["record_spans"][1][1]
    assert check(bam, "blk", 1, 1000) == (0, rows(reads, 0, 1, 1000))
    assert check(bam, "blk", 71, 80) == (0, rows(reads, 0, 71, 80))            # starts at read 1, in front of the seam


def test_stored_blocks(check, tmp_path):
    reads = _small_reads(8)
    bam = str(tmp_path / "stored.bam")
    write_bam(bam, [("st", 1000)], reads, block_payload=300, level=0)
    assert open(bam, "rb").read()[18] == 1                                     # BFINAL = 1, BTYPE = 00
    assert check(bam, "st", 1, 1000) == (0, rows(reads, 0, 1, 1000))


def test_empty_block_in_mid_file(check, tmp_path):
    """the 28-byte EOF block between two data blocks, once behind a record's last byte and once in the middle of a record"""
    reads = _small_reads(6)
    header = 12 + 4 + len("eof") + 1 + 4
    n = len(_record(reads[0], 0))
    src = str(tmp_path / "src.bam")
    info = write_bam(src, [("eof", 1000)], reads, block_payload=[header + 2 * n, n + n // 3, 60000])
    raw, bai = open(src, "rb").read(), open(src + ".bai", "rb").read()
    # one bin with one chunk, one linear window: only the chunk's end lies behind the blocks that move
    assert struct.unpack_from("<iiIi", bai, 4) == (1, 1, 4681, 1) and len(bai) == 8 + 4 + 8 + 16 + 4 + 8
    empty = _bgzf_block(b"")
    for k, at in enumerate(info["block_offsets"][1:3]):
        bam = str(tmp_path / ("eof%d.bam" % k))
        open(bam, "wb").write(raw[:at] + empty + raw[at:])
        end = struct.unpack_from("<Q", bai, 28)[0] + (len(empty) << 16)
        open(bam + ".bai", "wb").write(bai[:28] + struct.pack("<Q", end) + bai[36:])
        assert check(bam, "eof", 1, 1000) == (0, rows(reads, 0, 1, 1000))


@pytest.mark.parametrize("kind,text", [("fields_past_block_size", "check: alignment record shorter than its fields"),
                                       ("end_past_int32", "check: alignment at 805 runs past 2^31 - 1"),
                                       ("block_size_20", "check: bad alignment block size 20")])
def test_lying_records(check, kind, text):
    c = bamrecutil.lying_case(kind)
    status, out = check(c["bam"], "liar", 1, 3000)
    assert status == 1 and out[-1] == "error: " + text
    assert len(out) - 1 == 19 and all(int(line.split()[0]) < 805 for line in out[:-1])       # g00 .. g18 start in front of the liar


# ------------------------------------------------------------------------------------------------ indices
def test_damaged_bai(check, tmp_path):
    reads = _small_reads(6)
    bam = str(tmp_path / "idx.bam")
    write_bam(bam, [("idx", 1000)], reads)
    bai = open(bam + ".bai", "rb").read()
    assert check(bam, "idx", 1, 1000, bam + ".bai") == (0, rows(reads, 0, 1, 1000))
    damaged = {"cut_in_chunks": (bai[:30], "truncated BAI"), "cut_in_linear": (bai[:-3], "truncated BAI"), "cut_at_n_bin": (bai[:10], "truncated BAI"),
               "negative_n_bin": (bai[:8] + struct.pack("<i", -1) + bai[12:], "malformed BAI"),
               "negative_n_chunk": (bai[:16] + struct.pack("<i", -2) + bai[20:], "malformed BAI"),
               "no_magic": (b"BAJ\1" + bai[4:], "not a BAI index")}
    for name, (data, text) in damaged.items():
        path = str(tmp_path / (name + ".bai"))
        open(path, "wb").write(data)
        assert check(bam, "idx", 1, 1000, path) == (1, ["error: check: " + text]), name
    assert check(bam, "idx", 1, 1000, str(tmp_path / "none.bai"))[1][0].startswith("error: check: cannot open index")
    assert check(bam, "other", 1, 1000) == (1, ["error: check: contig other not in the BAM header"])


def test_tbi_query(check, tmp_path):
    """two sequences; the second one's chunks: the two of bin 4681 touch and merge, bin 4682's stands alone, the pseudo-bin 37450 is
    no chunk list, and everything in front of the first linear offset is cut off"""
    v = lambda coff, u: (coff << 16) | u
    names = b"chr1\0chr2\0"

    def ref(bins, linear):
        out = struct.pack("<i", len(bins))
        for b, chunks in bins:
            out += struct.pack("<Ii", b, len(chunks)) + b"".join(struct.pack("<QQ", *c) for c in chunks)
        return out + struct.pack("<i", len(linear)) + b"".join(struct.pack("<Q", x) for x in linear)
    chr1 = ref([(4681, [(v(0, 100), v(0, 900))])], [v(0, 100)])
    chr2 = ref([(0, [(v(500, 0), v(700, 10))]), (4681, [(v(1000, 20), v(1000, 800)), (v(1000, 800), v(2000, 5))]), (4682, [(v(3000, 0), v(3000, 64))]),
                (37450, [(v(1000, 20), v(3000, 64)), (3, 0)])], [v(1000, 20), v(3000, 0)])
    tbi = b"TBI\1" + struct.pack("<iiiiiiii", 2, 2, 1, 2, 0, ord("#"), 0, len(names)) + names + chr1 + chr2
    path = str(tmp_path / "x.tbi.inflated")
    open(path, "wb").write(tbi)
    assert check("tbi", path, "chr2") == (0, ["found 1", "%d %d" % (v(1000, 20), v(2000, 5)), "%d %d" % (v(3000, 0), v(3000, 64))])
    assert check("tbi", path, "chr1") == (0, ["found 1", "%d %d" % (v(0, 100), v(0, 900))])
    assert check("tbi", path, "chr") == (0, ["found 0"])
    open(path, "wb").write(tbi[:-5])
    assert check("tbi", path, "chr2") == (1, ["error: truncated BAI"])
    assert check("tbi", path, "chr1") == (0, ["found 1", "%d %d" % (v(0, 100), v(0, 900))])      # the cut lies behind chr1's part
    open(path, "wb").write(b"TBI\1" + struct.pack("<iiiiiiii", 2, 2, 1, 2, 0, ord("#"), 0, 4000) + names)
    assert check("tbi", path, "chr2") == (1, ["error: malformed tabix index"])
