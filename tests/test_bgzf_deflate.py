"""The BGZF coder's host restatement (csrc/deflate_host.h through cto_bgzf_deflate where = host): every block decodes with zlib to its
input, the block type is the cheapest of the three, the code lengths are valid and optimal where the limit allows, and the two writers
that use the coder (gen_contaminated_bam's mix, phase_tumor's haplotagged BAM) write files that differ from zlib's only in the
compressed bytes.  No GPU: tests/test_gpu_bgzf_deflate.py holds the kernels to these bytes."""
import gzip
import heapq
import struct
from fractions import Fraction

import numpy as np
import pytest

import bamutil
import contamutil as cu
import bgzfdeflateutil as du
import phaseutil as pu

from clairs_to_amd import bgzf
from clairs_to_amd import phase_tumor as pt

SHAPES = du.shapes()


def read(fn):
    with open(fn, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def coded():
    """name -> (blocks, sizes) of the host path, coded once"""
    return {name: bgzf.deflate_blocks(raw, where="host") for name, raw in SHAPES.items()}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_round_trip_and_type_choice(coded, name):
    raw = SHAPES[name]
    blocks, sizes = coded[name]
    du.check_blocks(raw, blocks, sizes)
    whole = blocks + du.EOF_BLOCK
    assert bgzf.deflate_bytes(raw, where="host") == whole
    assert gzip.decompress(whole) == raw
    for k, (payload, _, _, _) in enumerate(du.split_blocks(blocks)):
        bits, hist = du.block_sizes(raw[k * du.PAYLOAD:(k + 1) * du.PAYLOAD], "host")
        kind = (payload[0] >> 1) & 3
        assert bits[kind] == min(bits) and kind == bits.index(min(bits)), (name, k, bits)      # the cheapest, the first of equals
        assert len(payload) == (min(bits) + 7) // 8
        assert bits[0] == 8 * (len(raw[k * du.PAYLOAD:(k + 1) * du.PAYLOAD]) + 5)
        assert int(hist[256]) == 1


def test_a_whole_file_reads_back_through_the_package_reader(tmp_path):
    raw = SHAPES["2payload+7"]
    fn = tmp_path / "x.gz"
    fn.write_bytes(bgzf.deflate_bytes(raw, where="host"))
    stream, eof = cu.inflated(fn)
    assert eof and stream == raw
    assert cu.block_sizes(fn) == [du.PAYLOAD, du.PAYLOAD, 7, 0]
    assert bgzf.deflate_bytes(b"", where="host") == du.EOF_BLOCK


def test_what_the_shapes_are_there_for(coded):
    def toks(name, k=0):
        return du.tokens(du.split_blocks(coded[name][0])[k][0])
    kind, _, _ = toks("random")
    assert kind == 0                                                           # nothing to gain: stored
    kind, t, _ = toks("equal")
    assert kind == 2 and (258, 1) in t and {d for ln, d in t if ln} == {1}     # distance 1, chains of 258
    assert sum(ln or 1 for ln, _ in t) == du.PAYLOAD
    assert {d for ln, d in toks("period2")[1] if ln} == {2} and {d for ln, d in toks("period3")[1] if ln} == {3}
    _, t, _ = toks("far")
    assert not any(ln for ln, _ in t)                                          # 32769 back is out of reach
    bits, hist = du.block_sizes(SHAPES["far"], "host")
    assert int(hist[286:].sum()) == 0
    _, t, _ = toks("segment_end")
    assert [x for x in t if x[0]][:2] == [(10, du.SEG - 110), (30, du.SEG - 110)]          # cut at the segment's end, taken up again behind it
    assert t[-1] == (50, 3 * du.SEG - 50 - 900)                                # to the last byte of the block
    kind, t, (ll, dd) = toks("no_match")
    assert kind == 2 and not any(ln for ln, _ in t)
    assert sum(1 for x in dd if x) == 2 and sum(Fraction(1, 1 << x) for x in dd if x) == 1    # the forced pair: a complete distance code
    assert len(set(SHAPES["all_bytes"])) == 256 and {v for ln, v in toks("all_bytes")[1] if not ln} == set(range(256))


def test_the_crafted_block_uses_every_length_and_distance_code(coded):
    raw = SHAPES["crafted"]
    assert len(raw) <= du.PAYLOAD
    kind, t, _ = du.tokens(du.split_blocks(coded["crafted"][0])[0][0])
    assert kind == 2
    assert {ln for ln, _ in t if ln} >= set(range(3, 259))
    assert {d for ln, d in t if ln} >= set(du.DIST_EDGES)
    bits, hist = du.block_sizes(raw, "host")
    assert all(int(x) > 0 for x in hist[257:286]) and all(int(x) > 0 for x in hist[286:316])
    assert int(hist[:256].sum()) == sum(1 for ln, _ in t if not ln) and int(hist[257:286].sum()) == int(hist[286:].sum()) == sum(1 for ln, _ in t if ln)


# ------------------------------------------------------------------------------------------ code lengths
def huffman_cost_and_depth(freq):
    """sum f * depth and the greatest depth of a Huffman tree over the non-zero frequencies, ties broken towards the shallow tree"""
    heap = [(f, 0, [k]) for k, f in enumerate(freq) if f]
    heapq.heapify(heap)
    depth = {k: 0 for _, _, (k,) in heap}
    while len(heap) > 1:
        fa, da, a = heapq.heappop(heap)
        fb, db, b = heapq.heappop(heap)
        for k in a + b:
            depth[k] += 1
        heapq.heappush(heap, (fa + fb, max(da, db) + 1, a + b))
    return sum(freq[k] * d for k, d in depth.items()), max(depth.values())


def check_lengths(freq, max_bits, lens):
    used = [k for k, f in enumerate(freq) if f]
    assert all(0 <= x <= max_bits for x in lens)
    coded_syms = [k for k, x in enumerate(lens) if x]
    assert len(coded_syms) >= 2 and sum(Fraction(1, 1 << lens[k]) for k in coded_syms) == 1
    assert set(used) <= set(coded_syms)
    forced = sorted(set(coded_syms) - set(used))
    assert len(forced) == max(0, 2 - len(used)) and all(k < 3 for k in forced)
    if len(used) >= 2:
        cost, depth = huffman_cost_and_depth(freq)
        if depth <= max_bits:
            assert sum(freq[k] * lens[k] for k in used) == cost
    return coded_syms


CODE_CASES = {
    "fibonacci22_of_286": (du.fibonacci_freq(22, 286, stride=13), 15),
    "fibonacci19": (du.fibonacci_freq(19, 19), 7),
    "one_symbol_0": ([5] + [0] * 29, 15),
    "one_symbol_1": ([0, 9] + [0] * 28, 15),
    "one_symbol_late": ([0] * 200 + [3] + [0] * 85, 15),
    "none": ([0] * 30, 15),
    "two_symbols": ([0, 0, 0, 7, 0, 1] + [0] * 24, 15),
    "all_equal_286": ([3] * 286, 15),
    "all_equal_19": ([1] * 19, 7),
    "all_equal_30": ([2] * 30, 15),
    "skewed_286": ([1 + (k * k) % 97 + (40000 if k == 101 else 0) for k in range(286)], 15),
}


@pytest.mark.parametrize("name", sorted(CODE_CASES))
def test_code_lengths(name):
    freq, max_bits = CODE_CASES[name]
    lens = du.code_lengths(freq, max_bits, "host")
    check_lengths(freq, max_bits, lens)
    if name == "fibonacci22_of_286":
        assert sum(freq) == 46367 and huffman_cost_and_depth(freq)[1] == 21 and max(lens) == 15
    if name == "fibonacci19":
        assert max(lens) == 7
    if name == "two_symbols":
        assert [x for x in lens if x] == [1, 1]


# ------------------------------------------------------------------------------------------ the writers
@pytest.fixture(scope="module")
def bams(tmp_path_factory):
    """the `hand` and `sim` inputs of tests/test_gpu_contam.py's recipe, at level 6"""
    d = tmp_path_factory.mktemp("deflate_mix")
    sims = {s: pu.sim_case(s) for s in (7, 11)}
    t, n = str(d / "t.bam"), str(d / "n.bam")
    bamutil.write_bam(t, cu.HAND_REFS, cu.mix_reads("t"), block_payload=3000, level=6)
    bamutil.write_bam(n, cu.HAND_REFS, cu.mix_reads("n"), block_payload=3000, level=6)
    st, sn = str(d / "sim7.bam"), str(d / "sim11.bam")
    refs = [(pu.SIM_CTG, sims[7]["ref_len"])]
    bamutil.write_bam(st, refs, sims[7]["reads"], level=6)
    bamutil.write_bam(sn, refs, [dict(r, name="n" + r["name"]) for r in sims[11]["reads"]], level=6)
    return {"dir": d, "hand": dict(t=t, n=n, refs=cu.HAND_REFS, regions=[("c1", 1, 20000), ("c1", 30000, 70000), ("c2", 100, 30000)]),
            "sim": dict(t=st, n=sn, refs=refs, regions=[(pu.SIM_CTG, 1, 3000), (pu.SIM_CTG, 5000, 6000), (pu.SIM_CTG, 8900, 10 ** 6)])}


@pytest.mark.parametrize("which", ["hand", "sim"])
def test_mix_with_the_host_coder(bams, which, monkeypatch):
    from clairs_to_amd.gen_contaminated_bam import mix_bams
    from clairs_to_amd.realign_reads import bam_view
    monkeypatch.setenv("CTO_CONTAM_CHUNK_BYTES", "20000")                      # hand: several windows, bytes carried from one to the next
    b, d = bams[which], bams["dir"]
    out_z, out_h, out_0 = (str(d / ("%s_%s.bam" % (which, tag))) for tag in ("zlib", "host", "plain"))
    st_z, st_h, dst = {}, {}, {}
    res_0 = mix_bams(b["t"], b["n"], out_0, 600, 400, seed=2, where="host", host_threads=2)
    res_z = mix_bams(b["t"], b["n"], out_z, 600, 400, seed=2, where="host", host_threads=2, stats=st_z, deflate="zlib")
    res_h = mix_bams(b["t"], b["n"], out_h, 600, 400, seed=2, where="host", host_threads=2, stats=st_h, deflate="host", deflate_stats=dst)
    assert res_0 == res_z == res_h and st_z["n_chunks"] == st_h["n_chunks"] >= (4 if which == "hand" else 1)
    assert read(out_z) == read(out_0) and read(out_z + ".bai") == read(out_0 + ".bai")           # zlib is what the flag's absence gives
    stream_z, eof_z = cu.inflated(out_z)
    stream_h, eof_h = cu.inflated(out_h)
    assert eof_z and eof_h and stream_h == stream_z
    assert cu.block_sizes(out_h) == cu.block_sizes(out_z)
    assert read(out_h) != read(out_z)
    header, refs, t_recs = cu.read_bam(b["t"])
    _, _, n_recs = cu.read_bam(b["n"])
    merged = cu.merged_records(t_recs, n_recs, len(refs), 600, 400, 2)
    assert read(out_h + ".bai") == cu.expected_bai(out_h, header, len(refs), merged)
    for c, s, e in b["regions"]:
        rows = bam_view(out_z, c, s, e)
        assert bam_view(out_h, c, s, e) == rows
    assert sum(len(bam_view(out_z, c, s, e)) for c, s, e in b["regions"]) > 10
    n_blocks = len(cu.block_sizes(out_h)) - 1
    assert dst["n_blocks"] == n_blocks and dst["in_bytes"] == len(stream_h) == st_h["out_bytes"]
    assert dst["out_bytes"] == len(read(out_h)) - 28 and dst["stored"] + dst["fixed"] + dst["dynamic"] == n_blocks
    if which == "sim":
        assert dst["out_bytes"] < dst["in_bytes"]
    with pytest.raises(ValueError):
        mix_bams(b["t"], b["n"], out_h, 600, 400, where="host", deflate="gzip")


def test_mix_command_line_flag(bams, capsys):
    from clairs_to_amd.gen_contaminated_bam import main
    b, outs = bams["hand"], {}
    for tag, extra in (("none", []), ("zlib", ["--deflate", "zlib"]), ("host", ["--deflate", "host"])):
        od = str(bams["dir"] / ("cli_" + tag))
        main(["--tumor_bam_fn", b["t"], "--normal_bam_fn", b["n"], "--output_dir", od, "--tumor_purity", "0.7", "--where", "host", "--samtools_threads", "2",
              "--normal_bam_coverage", "10", "--tumor_bam_coverage", "10"] + extra)
        printed = capsys.readouterr().out
        assert "[INFO] BGZF deflate of the output: %s\n" % ("host" if tag == "host" else "zlib") in printed
        outs[tag] = (read(od + "/tumor_purity_0.7.bam"), read(od + "/tumor_purity_0.7.bam.bai"))
    assert outs["none"] == outs["zlib"]
    assert outs["host"][0] != outs["zlib"][0] and cu.inflated(bams["dir"] / "cli_host" / "tumor_purity_0.7.bam")[0] == gzip.decompress(outs["zlib"][0])


def bam_records(path):
    """[(virtual offset, record bytes)] of every alignment record, by a linear scan"""
    rd = pt.BgzfReader(path)
    head = rd.read(8)
    rd.read(struct.unpack_from("<i", head, 4)[0])
    for _ in range(struct.unpack("<i", rd.read(4))[0]):
        rd.read(struct.unpack("<i", rd.read(4))[0] + 4)
    out = []
    while True:
        v = rd.tell()
        h4 = rd.read(4)
        if len(h4) < 4:
            break
        out.append((v, rd.read(struct.unpack("<i", h4)[0])))
    rd.close()
    return out


def phase_cli(d, tag, extra, where="host"):
    from clairs_to_amd.__main__ import dispatch
    bam = str(d / tag / ("tumor_%s.bam" % pu.SIM_CTG))
    dispatch("phase_tumor", ["--tumor_bam_fn", str(d / "t.bam"), "--vcf_fn", str(d / (pu.SIM_CTG + ".vcf")), "--ctg_name", pu.SIM_CTG,
                             "--output_vcf_fn", str(d / tag / "phased.vcf.gz"), "--output_bam_fn", bam, "--where", where] + extra)
    return bam


def phase_inputs(d):
    case = pu.sim_case(7)
    pu.write_sim_bam(d / "t.bam", case)
    head = ("##fileformat=VCFv4.2\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n")
    (d / (pu.SIM_CTG + ".vcf")).write_text(head + "".join("%s\t%d\t.\t%s\t%s\t30\tPASS\t.\tGT:GQ:DP:AF\t0/1:30:40:0.4800\n" % (pu.SIM_CTG, p, r, a)
                                                          for p, r, a in case["sites"]))
    return case


def check_index(bam, case):
    """every chunk of the index starts and ends at a record boundary of the file, and the records they cover are all of them"""
    recs = bam_records(bam)
    starts = [v for v, _ in recs]
    ends = starts[1:] + [None]
    bai = read(bam + ".bai")
    assert bai[:4] == b"BAI\1" and struct.unpack_from("<i", bai, 4)[0] == 1
    n_bin, o, covered = struct.unpack_from("<i", bai, 8)[0], 12, 0
    for _ in range(n_bin):
        _, n_chunk = struct.unpack_from("<Ii", bai, o)
        o += 8
        for k in range(n_chunk):
            vb, ve = struct.unpack_from("<QQ", bai, o + 16 * k)
            i = starts.index(vb)
            j = i
            while ends[j] is not None and ends[j] != ve:
                j += 1
            covered += j - i + 1
        o += 16 * n_chunk
    assert covered == len(recs) == len(case["reads"])
    n_intv = struct.unpack_from("<i", bai, o)[0]
    lin = struct.unpack_from("<%dQ" % n_intv, bai, o + 4)
    assert n_intv > 0 and all(v in starts for v in lin if v) and list(lin) == sorted(lin)


def test_phase_tumor_with_the_host_coder(tmp_path, monkeypatch):
    case = phase_inputs(tmp_path)
    monkeypatch.setattr(pt.BatchBgzfWriter, "BATCH", 3)                        # several cto_bgzf_deflate calls for this small file
    plain, zl, host = phase_cli(tmp_path, "plain", []), phase_cli(tmp_path, "zlib", ["--deflate", "zlib"]), phase_cli(tmp_path, "host", ["--deflate", "host"])
    assert read(plain) == read(zl) and read(plain + ".bai") == read(zl + ".bai")
    assert read(host) != read(zl)
    rz, rh = bam_records(zl), bam_records(host)
    assert [r for _, r in rh] == [r for _, r in rz] and len(rh) == len(case["reads"])          # records and tags
    assert sum(b"HPi" in r for _, r in rh) > 10
    assert cu.inflated(host) == cu.inflated(zl) and cu.block_sizes(host) == cu.block_sizes(zl)
    assert len(cu.block_sizes(host)) > 5
    check_index(host, case)
    check_index(zl, case)
    # the same index rules: the two files' indices name the same records
    def named(bam):
        starts = {v: i for i, (v, _) in enumerate(bam_records(bam))}
        bai = read(bam + ".bai")
        n_bin, o, out = struct.unpack_from("<i", bai, 8)[0], 12, []
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", bai, o)
            out.append((b, [starts[struct.unpack_from("<Q", bai, o + 8 + 16 * k)[0]] for k in range(n_chunk)]))
            o += 8 + 16 * n_chunk
        n_intv = struct.unpack_from("<i", bai, o)[0]
        return out, [starts.get(v, -1) for v in struct.unpack_from("<%dQ" % n_intv, bai, o + 4)]
    assert named(host) == named(zl)
