"""The AF tallies' device path (csrc/aftally.hip) against the host path and the naive rules of tests/calafutil.py: exactly equal; only
the planted order-dependent loci leave the device; chunking changes nothing; a damaged block sends its chunk to the host path; the CLI
writes the reference's file (tests/golden/cal_af.json.gz) from either path."""
import ctypes as C
import shutil
import struct

import numpy as np
import pytest

from bamutil import _record
from calafutil import BLOCK_PAYLOAD, CHUNK_BYTES, LOW_MAX_DEPTH, OTHER_SKIP_LOCI, REFS, case, config_argv, contig_loci, expected, expected_host_loci, golden, write_vcfs

pytestmark = pytest.mark.gpu


def _tally(ctg, where, with_hp=True, max_depth=LOW_MAX_DEPTH, bam=None, stats=None):
    from clairs_to_amd.cal_af_distribution import allele_of, tally
    loci, ra = contig_loci(ctg)
    return tally(bam or case()["bam"], ctg, loci, [allele_of(r, a) for r, a in ra], with_hp=with_hp, max_depth=max_depth, where=where, stats=stats)


@pytest.mark.parametrize("with_hp", [True, False])
@pytest.mark.parametrize("ctg", [n for n, _ in REFS])
def test_device_equals_host_equals_naive(ctg, with_hp):
    """max_depth lowered to 16: on chrB exactly the planted loci go to the host path - three under a reference skip (not without the HP
    column), the deep one, the insertion allele of 70 bases; on chrA and chrC the four loci drawn under reference skips, and none without
    the HP column"""
    stats = {}
    dev = _tally(ctg, "device", with_hp, stats=stats)
    np.testing.assert_array_equal(dev, _tally(ctg, "host", with_hp))
    np.testing.assert_array_equal(dev, expected(ctg, with_hp, LOW_MAX_DEPTH))
    assert stats["fallback_chunks"] == 0 and stats["n_chunks"] == 1 and stats["n_blocks"] > 5
    assert stats["host_loci"] == expected_host_loci(ctg, with_hp, LOW_MAX_DEPTH)
    if ctg == "chrB":
        assert stats["host_loci"] == (5 if with_hp else 2)
    else:
        assert stats["host_loci"] == (OTHER_SKIP_LOCI if with_hp else 0)


def test_default_depth_cap_keeps_the_deep_locus_on_the_device():
    stats = {}
    dev = _tally("chrB", "device", True, max_depth=8000, stats=stats)
    np.testing.assert_array_equal(dev, expected("chrB", True, 8000))
    assert stats["host_loci"] == 4 and stats["fallback_chunks"] == 0


@pytest.mark.parametrize("with_hp", [True, False])
def test_device_chunks_do_not_change_the_tallies(monkeypatch, with_hp):
    monkeypatch.setenv("CTO_AF_CHUNK_BYTES", CHUNK_BYTES)
    stats, hstats = {}, {}
    dev = _tally("chrA", "device", with_hp, stats=stats)
    assert stats["n_chunks"] >= 3 and stats["fallback_chunks"] == 0
    np.testing.assert_array_equal(dev, expected("chrA", with_hp, LOW_MAX_DEPTH))
    np.testing.assert_array_equal(dev, _tally("chrA", "host", with_hp, stats=hstats))
    assert stats["n_reads_entered"] == hstats["n_reads_entered"] and stats["n_chunks"] == hstats["n_chunks"]
    assert stats["host_loci"] == expected_host_loci("chrA", with_hp, LOW_MAX_DEPTH)


@pytest.mark.parametrize("name", ["all_hp", "chrB_nohp"])
def test_cli_device_file_equals_host_file_equals_the_fixture(tmp_path, name):
    from clairs_to_amd.__main__ import dispatch
    cf = next(c for c in golden()["configs"] if c["name"] == name)
    write_vcfs(str(tmp_path))
    for where in ("device", "host"):
        dispatch("cal_af_distribution", config_argv(cf, str(tmp_path), tmp_path / (where + ".txt"), where))
    assert (tmp_path / "device.txt").read_bytes() == (tmp_path / "host.txt").read_bytes()
    assert (tmp_path / "device.txt").read_bytes() == cf["output"].encode()


def test_a_damaged_block_sends_the_chunk_to_the_host_path(tmp_path):
    """one corrupted payload byte in a BGZF block that chrA's byte range holds and chrA's reads do not (it belongs to the next contig):
    the device path declines the chunk (inflate status or CRC-32), the host path - which never opens that block - gives the tallies"""
    from clairs_to_amd._lib import check, lib
    c = case()
    raw = bytearray(open(c["bam"], "rb").read())
    offs, o = [], 0                                               # file offset of every BGZF block
    while o < len(raw):
        offs.append(o)
        o += struct.unpack_from("<H", raw, o + 16)[0] + 1
    header = 12 + sum(4 + len(n) + 1 + 4 for n, _ in REFS)
    first_b = header + sum(len(_record(r, r["ref"])) for r in c["reads"] if r["ref"] == 0)       # where the next contig's records start
    k = first_b // BLOCK_PAYLOAD + 2
    loci = contig_loci("chrA")[0]
    fb, fe = C.c_int64(), C.c_int64()
    check(lib.cto_bam_chunk_span(c["bam"].encode(), None, b"chrA", loci[0], loci[-1], C.byref(fb), C.byref(fe)))
    assert offs[k + 1] <= fe.value                                 # wholly inside what the device inflates for chrA
    raw[offs[k] + 18 + 7] ^= 0x5a
    bad = str(tmp_path / "bad.bam")
    open(bad, "wb").write(bytes(raw))
    shutil.copy(c["bam"] + ".bai", bad + ".bai")
    stats = {}
    got = _tally("chrA", "device", bam=bad, stats=stats)
    assert stats["fallback_chunks"] == 1 and stats["n_chunks"] == 1 and stats["host_loci"] == 0
    np.testing.assert_array_equal(got, expected("chrA", True, LOW_MAX_DEPTH))
    np.testing.assert_array_equal(got, _tally("chrA", "host", bam=bad))
