"""The device record front end (csrc/bam_records.h: k_crc32_blocks, k_linearise, k_chain, record_cigar, parse_record) through both of
its consumers - the allele counter and the column pile-up - on the files of tests/bamrecutil.py: auxiliary areas of every layout
around CG:B,I, BGZF blocks at the seams of the CRC-32 slices, fixed fields at their gates, records whose fields lie.  The device is
held to the host path and to the naive rules, exactly, and may not hand a valid chunk to the host (fallback_chunks == 0); the host
side of the same expectations is tests/test_bam_records.py."""
import numpy as np
import pytest

import bamrecutil as U
from allelecountutil import PARAMS
from bamutil import effective_cigar
from test_bam_reader import _pack_arrays
from test_gpu_pileup import _device_arrays

pytestmark = pytest.mark.gpu

PACK_ARRAYS = ("col_pos", "col_ref", "col_off", "key_off", "entries", "key_meta", "key_group")


def _count(bam, ctg, loci, params, where, stats=None):
    from clairs_to_amd.allele_counter import count_alleles
    bq, mq, f, F = params
    return count_alleles(bam, ctg, loci, min_bq=bq, min_mq=mq, req_flags=f, excl_flags=F, where=where, stats=stats)


def _device_equals_host_equals_naive(bam, ctg, loci, params, want, entered, named_reads=()):
    stats, hstats = {}, {}
    dev = _count(bam, ctg, loci, params, "device", stats=stats)
    host = _count(bam, ctg, loci, params, "host", stats=hstats)
    assert np.array_equal(dev, host), "device against host: " + U.blame(loci, dev, host, named_reads)
    assert np.array_equal(dev, want), "device against naive: " + U.blame(loci, dev, want, named_reads)
    assert stats["fallback_chunks"] == 0 and stats["n_chunks"] == 1              # the host path did not stand in
    assert stats["n_reads_entered"] == hstats["n_reads_entered"] == entered
    return stats


@pytest.fixture(scope="module")
def dp():
    from clairs_to_amd.bgzf import DevicePileup
    return DevicePileup()


def _device_pack(dp, bam, ctg, start, end, ref_seq):
    """(arrays, fallback) of DevicePileup.pileup; arrays is None with fallback"""
    import torch
    from clairs_to_amd._lib import lib
    pv, lite, fallback = dp.pileup(bam, None, ctg, start, end, ref_seq, 1, torch.device("cuda:0"))
    if fallback:
        return None, True
    got = _device_arrays(pv, lite)
    lib.cto_pack_free(lite)
    return got, False


def _device_pack_equals_host(dp, bam, ctg, start, end, ref_seq, what):
    from clairs_to_amd.pack import ColumnPack
    want = _pack_arrays(ColumnPack.from_bam(bam, ctg, start, end, ref_seq, 1))
    got, fallback = _device_pack(dp, bam, ctg, start, end, ref_seq)
    assert not fallback, what
    for k in PACK_ARRAYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s: %s" % (what, k))
    assert got["keys"] == want["keys"], what
    return len(want["col_pos"])


# ------------------------------------------------------------------------------------------------ the aux walk
@pytest.mark.parametrize("params", sorted(U.AUX_PARAMS))
def test_aux_layouts_device_counts(params):
    c = U.aux_case()
    want, entered = U.aux_expected(params)
    _device_equals_host_equals_naive(c["bam"], U.AUX_CTG, c["loci"], U.AUX_PARAMS[params], want, entered, [(n, r) for n, r, _ in c["layouts"]])


def test_aux_layouts_device_pileup(dp):
    """every layout's own 200 bases: the host reader's pack where the read's effective CIGAR has no reference skip; where the
    placeholder stands the read enters as <l_seq>S<ref_len>N and the call reports `fallback`, never a pack.  (field_k_not_lseq keeps
    an N too, but its field does not consume l_seq bases: the record is skipped by both, no fallback.)"""
    c = U.aux_case()
    n_fallback = 0
    for name, r, taken in c["layouts"]:
        eff = effective_cigar(r)
        start, end = U.aux_region(r)
        if "N" in {op for op, _ in eff} and U.query_len_of(eff) == len(r["seq"]):
            got, fallback = _device_pack(dp, c["bam"], U.AUX_CTG, start, end, c["ref_seq"])
            assert fallback and got is None, name
            n_fallback += 1
        else:
            assert _device_pack_equals_host(dp, c["bam"], U.AUX_CTG, start, end, c["ref_seq"], name) > 20, name
    assert n_fallback == 8


# ------------------------------------------------------------------------------------------------ blocks at the slice seams
def test_seam_blocks_device(dp):
    c = U.seams_case()
    fb, fe = U.chunk_span(c["bam"], "seams", c["loci"])
    assert fb == c["seam_blocks"][0] and c["seam_blocks"][1] <= fe       # from the one-byte block on: every seam block is inflated and checked
    stats = _device_equals_host_equals_naive(c["bam"], "seams", c["loci"], PARAMS["verdict"], c["want"],
                                             U.naive_entered(c["reads"], 0, c["loci"], *PARAMS["verdict"]))
    assert stats["n_blocks"] >= c["n_data_blocks"]                       # every block behind the header's (the empty last one may count)
    assert _device_pack_equals_host(dp, c["bam"], "seams", 1, c["length"], c["ref_seq"], "seams") > 15000


def test_stored_blocks_device(dp):
    """the undamaged file of stored blocks, the full 64-slice block in its span: nothing declined"""
    c = U.stored_case()
    stats = _device_equals_host_equals_naive(c["bam"], "c0", c["loci"], PARAMS["verdict"], c["want"], c["entered"])
    assert stats["n_blocks"] == 2 and stats["inflated_bytes"] > U.STORED_SIZE
    assert _device_pack_equals_host(dp, c["bam"], "c0", 1, 3000, c["ref_seq"], "stored") >= 1000     # 40 reads in a row, each over 25 reference bases or more


@pytest.mark.parametrize("flip", sorted(U.STORED_FLIPS) + ["trailer_crc"])
def test_one_flipped_byte_in_any_slice_fails_the_crc(dp, flip):
    """one byte of the 64-slice stored block XORed (last of slice 0, first of slice 1, inside slice 31, first of slice 63, the block's
    last), or one bit of the trailer's CRC field: inflate succeeds (bamrecutil.stored_case asserts it with zlib), so only
    k_crc32_blocks can object - and a kernel that left any one slice out of the chain would not.  The block lies in c0's byte range
    and holds none of c0's records: the chunk goes to the host path, which gives the counts."""
    from clairs_to_amd._lib import CtoError
    c = U.stored_case()
    bam = c["copies"][flip]
    fb, fe = U.chunk_span(bam, "c0", c["loci"])
    assert fb <= c["block1"][0] and c["block1"][1] <= fe                         # wholly inside what the device inflates for c0
    stats = {}
    got = _count(bam, "c0", c["loci"], PARAMS["verdict"], "device", stats=stats)
    assert stats["fallback_chunks"] == 1 and stats["n_chunks"] == 1
    np.testing.assert_array_equal(got, _count(bam, "c0", c["loci"], PARAMS["verdict"], "host"))
    np.testing.assert_array_equal(got, c["want"])
    assert stats["n_reads_entered"] == c["entered"]
    with pytest.raises(CtoError, match="CRC-32"):                                # the pile-up declines the copy as well
        _device_pack(dp, bam, "c0", 1, 3000, c["ref_seq"])


# ------------------------------------------------------------------------------------------------ fixed fields, the chain
@pytest.mark.parametrize("params", sorted(U.AUX_PARAMS))
@pytest.mark.parametrize("region", sorted(U.FIELD_REGIONS))
def test_fixed_field_gates_device(region, params):
    c = U.fields_case()
    ri, loci = U.FIELD_REGIONS[region]
    want, entered = U.fields_expected(region, params)
    named = [(r["name"][:20], r) for r in c["reads"] if r["ref"] == ri and r["pos"] >= 0]
    _device_equals_host_equals_naive(c["bam"], U.FIELD_REFS[ri][0], loci, U.AUX_PARAMS[params], want, entered, named)


def _outcome(call):
    from clairs_to_amd._lib import CtoError
    try:
        return "counts", call()
    except CtoError as e:
        return "error", str(e).split(":")[0]


@pytest.mark.parametrize("kind", U.LYING)
def test_lying_records_device(dp, kind):
    """one record whose fields lie among good ones: the device call does what the host call does with the file - the same error code, or
    the same counts with the chunk declined - and never succeeds with other counts.  (The guards decline these records from their
    fixed fields alone: need <= block_size in parse_record, block_size >= 32 and the record inside the stream in k_chain.)"""
    from clairs_to_amd._lib import CtoError
    c = U.lying_case(kind)
    stats = {}
    host = _outcome(lambda: _count(c["bam"], "liar", c["loci"], PARAMS["verdict"], "host"))
    dev = _outcome(lambda: _count(c["bam"], "liar", c["loci"], PARAMS["verdict"], "device", stats=stats))
    assert dev[0] == host[0]
    if host[0] == "error":
        assert dev[1] == host[1] == "clairsto_amd error -1"
    else:
        np.testing.assert_array_equal(dev[1], host[1])
        assert stats["fallback_chunks"] == 1
    with pytest.raises(CtoError, match="error -1:"):                             # as the host reader of the pile-up does
        _device_pack(dp, c["bam"], "liar", 1, 3000, c["ref_seq"])
