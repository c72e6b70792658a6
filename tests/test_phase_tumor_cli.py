"""phase_tumor --where host, end to end on a simulated long-read BAM (tests/golden/hapsim.py, seed 7): the phased VCF, the haplotagged
BAM and its index, read back by this package's own BAM readers, and haplotype_filtering on the two outputs.  No GPU."""
import gzip
import struct

import pytest

import haputil
import phaseutil as pu
from conftest import load_json_gz

from clairs_to_amd import phase_tumor as pt

HEAD = ("##fileformat=VCFv4.2\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
        "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n")


def input_vcf(case):
    """the sites as select_hetero_snp_for_phasing hands them over, an indel row and a row of another contig among them"""
    rows = ["%s\t%d\t.\t%s\t%s\t%d\tPASS\t.\tGT:GQ:DP:AF\t%s:%d:40:0.4800\n" % (pu.SIM_CTG, p, r, a, 10 + k % 7, "0/1" if k % 3 else "1/0", 10 + k % 7)
            for k, (p, r, a) in enumerate(case["sites"])]
    rows.insert(5, "%s\t%d\t.\tAT\tA\t30\tPASS\t.\tGT:GQ:DP:AF\t0/1:30:40:0.5000\n" % (pu.SIM_CTG, case["sites"][4][0] + 1))
    rows.insert(0, "chr0\t77\t.\tA\tC\t30\tPASS\t.\tGT:GQ:DP:AF\t0/1:30:40:0.5000\n")
    return HEAD + "".join(rows)


def run_cli(d, where, tag):
    argv = ["--tumor_bam_fn", str(d / "t.bam"), "--vcf_fn", str(d / "vcf" / (pu.SIM_CTG + ".vcf")), "--ctg_name", pu.SIM_CTG,
            "--output_vcf_fn", str(d / tag / "phased_vcf_output" / ("tumor_phased_%s.vcf.gz" % pu.SIM_CTG)),
            "--output_bam_fn", str(d / tag / "phased_bam_output" / ("tumor_%s.bam" % pu.SIM_CTG)), "--where", where]
    from clairs_to_amd.__main__ import dispatch
    dispatch("phase_tumor", argv)
    return argv[7], argv[9]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("phase_cli")
    case = pu.sim_case(7)
    info = pu.write_sim_bam(d / "t.bam", case)
    (d / "vcf").mkdir()
    (d / "vcf" / (pu.SIM_CTG + ".vcf")).write_text(input_vcf(case))
    vcf, bam = run_cli(d, "host", "host")
    res = pt.phase_reads(str(d / "t.bam"), pu.SIM_CTG, [s[0] for s in case["sites"]], [s[1] for s in case["sites"]], [s[2] for s in case["sites"]],
                         where="host")
    return dict(dir=d, case=case, info=info, vcf=vcf, bam=bam, res=res)


def records(path):
    """[(virtual offset, record bytes)] of every alignment record of a BAM, by a linear scan"""
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


def split_record(rec):
    l_name, n_cig, l_seq = rec[8], struct.unpack_from("<H", rec, 12)[0], struct.unpack_from("<i", rec, 16)[0]
    a0 = 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq
    return rec[:a0], rec[a0:]


def test_phased_vcf_keeps_every_row(run):
    want = input_vcf(run["case"]).splitlines(True)
    with gzip.open(run["vcf"], "rt") as f:
        got = f.readlines()
    ps_head = [r for r in got if r.startswith("##FORMAT=<ID=PS,Number=1,Type=Integer,")]
    assert len(ps_head) == 1 and got.index(ps_head[0]) == next(i for i, r in enumerate(got) if r.startswith("#CHROM")) - 1
    got.remove(ps_head[0])
    assert len(got) == len(want)
    site_of = {s[0]: k for k, s in enumerate(run["case"]["sites"])}
    n_phased = 0
    for w, g in zip(want, got):
        c, e = g.rstrip("\n").split("\t"), w.rstrip("\n").split("\t")
        k = site_of.get(int(e[1])) if not w.startswith("#") and e[0] == pu.SIM_CTG and len(e[3]) == 1 else None
        if k is None or run["res"]["phase"][k] < 0:
            assert g == w                                                 # headers, other contigs, indels, unphased sites: as they were
            continue
        n_phased += 1
        ph = int(run["res"]["phase"][k])
        assert c[:8] == e[:8] and c[8] == e[8] + ":PS"
        assert c[9].split(":") == ["%d|%d" % (ph, 1 - ph)] + e[9].split(":")[1:] + [str(int(run["res"]["ps"][k]))]
    assert n_phased == int((run["res"]["phase"] >= 0).sum()) >= 20


def test_bam_records_keep_their_bytes(run):
    src, out = records(str(run["dir"] / "t.bam")), records(run["bam"])
    assert len(src) == len(out) == len(run["case"]["reads"])
    tag_of = {int(v): (int(h), int(p)) for v, h, p in zip(run["res"]["voff"], run["res"]["hp"], run["res"]["read_ps"])}
    assert [v for v, _ in src] == pu.voffs_of(run["info"])
    n_stale = n_tagged = 0
    for (v, a), (_, b) in zip(src, out):
        fa, xa = split_record(a)
        fb, xb = split_record(b)
        assert fa == fb                                                   # fixed fields, name, CIGAR, SEQ, QUAL
        n_stale += b"HP" in xa
        hp, ps = tag_of.get(v, (0, 0))
        kept = pt.strip_tags(xa)
        assert b"HP" not in kept
        assert xb == kept + (b"HPi" + struct.pack("<i", hp) + b"PSi" + struct.pack("<i", ps) if hp else b"")
        n_tagged += hp != 0
    assert n_stale > 200 and n_tagged > 350


def hp_by_read(bam, lo, hi, positions):
    from clairs_to_amd.haplotype_filtering import HapJob
    with HapJob.from_bam(bam, pu.SIM_CTG, lo, hi, haputil.merged_intervals(positions), where="host") as j:
        cols = haputil.job_columns(j.view())
    out = {}
    for _, rows, _ in cols:
        for r in rows:
            assert out.setdefault(r[0], r[5]) == r[5]
    return cols, out


def test_output_bam_shows_the_tags_through_hap_windows(run):
    case, res = run["case"], run["res"]
    positions = list(range(1, case["ref_len"], 150))                     # every read is at least 300 bases long
    _, seen = hp_by_read(run["bam"], 1, case["ref_len"], positions)
    voff = pu.voffs_of(run["info"])
    tag_of = {int(v): int(h) for v, h in zip(res["voff"], res["hp"])}
    n = 0
    for i, r in enumerate(case["reads"]):
        key = "%s_%d" % (r["name"], 1 if r["flag"] & 16 else 0)
        if r["mapq"] < 20:
            assert key not in seen
            continue
        want = tag_of.get(voff[i], 0)
        assert seen[key] == (str(want) if want else "*"), r["name"]
        n += 1
    assert n > 350
    # the input's own tags were the simulation's haplotypes, on four reads of five: the new ones replaced them
    assert sum(1 for i, r in enumerate(case["reads"]) if b"HP" not in r["aux"] and tag_of.get(voff[i], 0)) > 50


def test_bai_fetches_what_a_linear_scan_finds(run):
    case = run["case"]
    lo, hi = 4001, 4600
    positions = list(range(lo, hi + 1, 50))
    cols, _ = hp_by_read(run["bam"], lo, hi, positions)
    assert [c[0] for c in cols] == positions
    out = records(run["bam"])
    for pos, rows, _ in cols:
        want = []
        for _, rec in out:
            p, l_name, mapq, n_cig, flag = struct.unpack_from("<i", rec, 4)[0], rec[8], rec[9], struct.unpack_from("<H", rec, 12)[0], struct.unpack_from("<H", rec, 14)[0]
            rlen = sum(c >> 4 for c in struct.unpack_from("<%dI" % n_cig, rec, 32 + l_name) if (c & 15) in (0, 2, 3, 7, 8))
            if mapq >= 20 and not (flag & 2316) and p < pos <= p + rlen:
                want.append("%s_%d" % (rec[32:32 + l_name - 1].decode(), 1 if flag & 16 else 0))
        assert [r[0] for r in rows] == want, pos
    # and the index itself: the bins are the records' own
    bai = open(run["bam"] + ".bai", "rb").read()
    assert bai[:4] == b"BAI\1" and struct.unpack_from("<i", bai, 4)[0] == 1
    n_bin = struct.unpack_from("<i", bai, 8)[0]
    bins, o = set(), 12
    for _ in range(n_bin):
        b, n_chunk = struct.unpack_from("<Ii", bai, o)
        bins.add(b)
        o += 8 + 16 * n_chunk
    assert bins == {struct.unpack_from("<H", rec, 10)[0] for _, rec in out}
    assert struct.unpack_from("<i", bai, o)[0] == (case["ref_len"] - 1) // 16384 + 1


def test_haplotype_filtering_runs_on_the_outputs(run, tmp_path):
    from clairs_to_amd.haplotype_filtering import haplotype_filter
    g = load_json_gz("hapfilter.json.gz")
    haputil.write_inputs(tmp_path, pu.SIM_CTG, g["ref"], g["germline_vcf"], g["modes"]["snv"]["pileup_vcf"])
    prefix = run["bam"][:-len(pu.SIM_CTG + ".bam")]                      # phased_bam_output/tumor_
    res = haplotype_filter(haputil.stage_args(tmp_path, pu.SIM_CTG, prefix, "snv", "out.vcf", "host", germline_vcf_fn=run["vcf"]))
    assert len(res) >= 20 and (tmp_path / "out.vcf").read_text().count("\n") > 20


def test_parser_and_help():
    a = pt.build_parser().parse_args(["--tumor_bam_fn", "t.bam", "--vcf_fn", "c.vcf", "--ctg_name", "c", "--output_vcf_fn", "o.vcf.gz", "--output_bam_fn", "o.bam"])
    assert (a.min_mq, a.link_span, a.where, a.bai_fn) == (20, 8, None, None)
    assert "No tabix index is written" in " ".join(pt.build_parser().format_help().split())
    with pytest.raises(SystemExit):
        pt.main(["--tumor_bam_fn", "t.bam"])
