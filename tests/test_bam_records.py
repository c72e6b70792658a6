"""The host twins of the device record front end (csrc/bam.cpp: resolve_cg_tag, the fixed-field gates of the two readers) on the files
of tests/bamrecutil.py, against the naive rules: auxiliary areas of every layout around CG:B,I, blocks at the CRC-32 slice seams,
fixed fields at their gates, records whose fields lie.  tests/test_gpu_bam_records.py holds the device to the same expectations.
PARITY UNPINNED against htslib (absent): the walk rules are the SAM specification's as bamutil.effective_cigar restates them."""
import numpy as np
import pytest

import bamrecutil as U
from allelecountutil import BLOCK_PAYLOAD, PARAMS, REFS, make_reads_and_loci
from bamutil import effective_cigar, mpileup_rows, write_bam
from test_bam_reader import _assert_same, _pack_arrays, _random_reads


def _host(bam, ctg, loci, params, stats=None):
    from clairs_to_amd.allele_counter import count_alleles
    bq, mq, f, F = params
    return count_alleles(bam, ctg, loci, min_bq=bq, min_mq=mq, req_flags=f, excl_flags=F, where="host", stats=stats)


def _host_pack_equals_naive(bam, reads, ref_index, ctg, start, end, ref_seq):
    from clairs_to_amd.pack import ColumnPack
    text = mpileup_rows(U.effective_reads(reads), ref_index, ctg, start, end, ref_seq=ref_seq, ref_start=1)
    want = ColumnPack.from_mpileup(text, ref_seq, 1)
    _assert_same(_pack_arrays(ColumnPack.from_bam(bam, ctg, start, end, ref_seq, 1)), _pack_arrays(want))
    return want.n_cols


# ------------------------------------------------------------------------------------------------ the writer
def test_the_old_call_form_writes_the_same_bytes(tmp_path):
    """the options the writer gained change nothing for a caller that does not use them: digests taken before they were added (the
    second of each pair does not depend on the zlib build: inflated blocks, the index by block number)"""
    import zlib
    reads, _ = make_reads_and_loci()
    a = str(tmp_path / "a.bam")
    write_bam(a, REFS, reads, block_payload=BLOCK_PAYLOAD)
    b = str(tmp_path / "b.bam")
    write_bam(b, [("chrA", 40000), ("chrB", 3000)], _random_reads(np.random.default_rng(1), 300, [40000, 3000], paired_frac=0.3))
    da, db = U.bam_digests(a), U.bam_digests(b)
    assert da[1] == "6cf7b4bd18ff33efdb003021cc8589dd4a5d4ce1551617bbc82ae2c6ef3795da"
    assert db[1] == "873e71cc2a5e21185b62906da3dc0157e537dcd20dbfd4580d930bd24cdeb636"
    if zlib.ZLIB_RUNTIME_VERSION == "1.2.11":               # the compressed bytes are that build's
        assert da[0] == "07429d9a7c3928701f48112756c9f13401e12e0aa1ea1f40613b6c374f9c9ff8"
        assert db[0] == "2ecfa03c244d9f5c518f65b4f8f2d8528108b89381fe82f621e9c16509041e6f"
    else:                                                   # another compressor: at least the same bytes from the same call, twice
        again = str(tmp_path / "again.bam")
        write_bam(again, REFS, reads, block_payload=BLOCK_PAYLOAD)
        assert U.bam_digests(again) == da


def test_effective_cigar_on_every_layout():
    """the restatement says of every layout what the layout was built to be: the tag's operations, or the field"""
    c = U.aux_case()
    assert len(c["layouts"]) == 49 and len({n for n, _, _ in c["layouts"]}) == 49
    for name, r, taken in c["layouts"]:
        eff = effective_cigar(r)
        assert eff == (r["cigar"] if taken else r["cigar_field"]), name
        assert 40 <= len(r["seq"]) <= 62 and len(r["cigar"]) >= 5 and {"I", "D"} <= {op for op, _ in r["cigar"]}, name
        assert "N" not in {op for op, _ in r["cigar"]}, name
    # the writer's own fixed fields, as every other test file has them
    plain = dict(c["reads"][3])
    assert plain.get("cg_tag") and effective_cigar(plain) == plain["cigar"]
    assert effective_cigar(dict(plain, cg_tag=False)) == plain["cigar"]


# ------------------------------------------------------------------------------------------------ the aux walk
@pytest.mark.parametrize("params", sorted(U.AUX_PARAMS))
def test_aux_layouts_host_counts_equal_naive(params):
    c = U.aux_case()
    want, entered = U.aux_expected(params)
    stats = {}
    got = _host(c["bam"], U.AUX_CTG, c["loci"], U.AUX_PARAMS[params], stats=stats)
    assert np.array_equal(got, want), U.blame(c["loci"], got, want, [(n, r) for n, r, _ in c["layouts"]])
    assert stats["n_reads_entered"] == entered and stats["n_chunks"] == 1
    assert want.sum() > 1000 and entered >= 2 * 49 - 2


def test_aux_layouts_host_pack_equals_naive():
    """the column pile-up's reader resolves the same CIGARs: the whole contig, then every layout's own region (where a placeholder
    stands the read is one long reference skip and contributes no column)"""
    c = U.aux_case()
    assert _host_pack_equals_naive(c["bam"], c["reads"], 0, U.AUX_CTG, 1, c["length"], c["ref_seq"]) > 3000
    for name, r, taken in c["layouts"]:
        start, end = U.aux_region(r)
        try:
            _host_pack_equals_naive(c["bam"], c["reads"], 0, U.AUX_CTG, start, end, c["ref_seq"])
        except AssertionError as e:
            raise AssertionError("layout %s: %s" % (name, e))


# ------------------------------------------------------------------------------------------------ blocks at the slice seams
def test_seam_blocks_host():
    c = U.seams_case()
    fb, fe = U.chunk_span(c["bam"], "seams", c["loci"])
    assert fb <= c["seam_blocks"][0] and c["seam_blocks"][1] <= fe       # every seam block is among what the device would inflate
    stats = {}
    np.testing.assert_array_equal(_host(c["bam"], "seams", c["loci"], PARAMS["verdict"], stats=stats), c["want"])
    assert c["want"].sum() > 3000
    assert _host_pack_equals_naive(c["bam"], c["reads"], 0, "seams", 1, c["length"], c["ref_seq"]) > 15000


def test_stored_blocks_host():
    """the host reader takes stored blocks, and never opens the damaged block of the copies: c0's records end in front of it"""
    c = U.stored_case()
    assert sorted(c["copies"]) == sorted(list(U.STORED_FLIPS) + ["trailer_crc"])
    for bam in [c["bam"]] + sorted(c["copies"].values()):
        stats = {}
        np.testing.assert_array_equal(_host(bam, "c0", c["loci"], PARAMS["verdict"], stats=stats), c["want"], err_msg=bam)
        assert stats["n_reads_entered"] == c["entered"] == 40
    assert c["want"].sum() > 300
    from clairs_to_amd._lib import CtoError
    from clairs_to_amd.allele_counter import count_alleles
    with pytest.raises(CtoError, match="CRC-32"):                       # c1's records do need the block
        count_alleles(c["copies"]["slice31"], "c1", [100, 29000], where="host")


# ------------------------------------------------------------------------------------------------ fixed fields, the chain
@pytest.mark.parametrize("params", sorted(U.AUX_PARAMS))
@pytest.mark.parametrize("region", sorted(U.FIELD_REGIONS))
def test_fixed_field_gates_host(region, params):
    c = U.fields_case()
    ri, loci = U.FIELD_REGIONS[region]
    want, entered = U.fields_expected(region, params)
    stats = {}
    got = _host(c["bam"], U.FIELD_REFS[ri][0], loci, U.AUX_PARAMS[params], stats=stats)
    named = [(r["name"][:20], r) for r in c["reads"] if r["ref"] == ri and r["pos"] >= 0]
    assert np.array_equal(got, want), U.blame(loci, got, want, named)
    assert stats["n_reads_entered"] == entered


def test_the_fixed_field_case_holds_what_it_is_meant_to():
    """said of the expectation itself: which of the edge reads enter the region's pile-up, and that the gates can show"""
    c = U.fields_case()
    by_name = {r["name"]: r for r in c["reads"]}
    enters = lambda name, region: U.naive_entered([by_name[name]], *U.FIELD_REGIONS[region], 0, 0, 0, 0)
    assert [enters(n, "f1") for n in ("ends_before_first", "ends_on_first", "starts_on_last", "starts_behind_last")] == [0, 1, 1, 0]
    assert [enters(n, "f1") for n in ("l_seq_1", "l_seq_2", "l_seq_3", "", "n" * 254, "mapq_255")] == [1] * 6
    assert [enters(n, "f1") for n in ("l_seq_0", "l_seq_0_del", "no_cigar")] == [0, 0, 0]
    assert enters("pos_minus_one", "f1_head") == 0 and enters("head", "f1_head") == 1
    # let in at its position, the record without one would cover the contig's first loci
    assert U.naive_entered([dict(by_name["pos_minus_one"], pos=0)], *U.FIELD_REGIONS["f1_head"], 0, 0, 0, 0) == 1
    assert U.fields_expected("f1", "verdict")[0][0].sum() >= 1 and U.fields_expected("f1_head", "verdict")[0].sum() >= 10
    assert sum(r["ref"] == -1 for r in c["reads"]) == 12 and c["reads"][-1]["ref"] == -1


def test_lying_records_host():
    """a record that needs more bytes than its block_size, one that ends past 2^31 - 1, one of 20 bytes: both host readers refuse the
    file with CTO_EINVAL (-1) once the scan reaches the record"""
    from clairs_to_amd._lib import CtoError
    from clairs_to_amd.pack import ColumnPack
    for kind in U.LYING:
        c = U.lying_case(kind)
        with pytest.raises(CtoError, match="error -1:"):
            _host(c["bam"], "liar", c["loci"], PARAMS["verdict"])
        with pytest.raises(CtoError, match="error -1:"):
            ColumnPack.from_bam(c["bam"], "liar", 1, 3000, c["ref_seq"], 1)
        # the reads in front of the record are counted when the region ends in front of it
        assert _host(c["bam"], "liar", [p for p in c["loci"] if p < 700], PARAMS["verdict"]).sum() > 100
