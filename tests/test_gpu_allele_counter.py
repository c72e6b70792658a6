"""The allele counter's device path (csrc/allelecount.hip) against its host path and the naive rules of tests/allelecountutil.py:
exactly equal, no chunk declined; a damaged block sends its chunk to the host path."""
import ctypes as C
import os
import shutil
import struct

import numpy as np
import pytest

from allelecountutil import BLOCK_PAYLOAD, CHUNK_BYTES, PARAMS, REFS, case, expected, loci_file_lines, naive_counts
from bamutil import _record, write_bam

pytestmark = pytest.mark.gpu


def _count(ctg, params, where, bam=None, stats=None):
    from clairs_to_amd.allele_counter import count_alleles
    bq, mq, f, F = PARAMS[params]
    c = case()
    return count_alleles(bam or c["bam"], ctg, c["loci"][ctg], min_bq=bq, min_mq=mq, req_flags=f, excl_flags=F, where=where, stats=stats)


@pytest.mark.parametrize("params", sorted(PARAMS))
@pytest.mark.parametrize("ctg", [n for n, _ in REFS])
def test_device_equals_host_equals_naive(ctg, params):
    stats = {}
    dev = _count(ctg, params, "device", stats=stats)
    np.testing.assert_array_equal(dev, _count(ctg, params, "host"))
    np.testing.assert_array_equal(dev, expected(ctg, params))
    assert stats["fallback_chunks"] == 0 and stats["n_chunks"] == 1 and stats["n_blocks"] > 10


@pytest.mark.parametrize("params", ["verdict", "defaults"])
def test_device_chunks_do_not_change_the_counts(monkeypatch, params):
    monkeypatch.setenv("CTO_ALLELE_CHUNK_BYTES", CHUNK_BYTES)
    stats, hstats = {}, {}
    dev = _count("chrA", params, "device", stats=stats)
    assert stats["n_chunks"] >= 3 and stats["fallback_chunks"] == 0
    np.testing.assert_array_equal(dev, expected("chrA", params))
    np.testing.assert_array_equal(dev, _count("chrA", params, "host", stats=hstats))
    assert stats["n_reads_entered"] == hstats["n_reads_entered"] and stats["n_chunks"] == hstats["n_chunks"]


def test_cli_device_table_equals_host_table(tmp_path):
    from clairs_to_amd.__main__ import dispatch
    loci_fn = tmp_path / "loci.txt"
    loci_fn.write_text("\n".join(loci_file_lines()) + "\n")
    for where in ("device", "host"):
        dispatch("allele_counter", ["-b", case()["bam"], "-l", str(loci_fn), "-o", str(tmp_path / (where + ".txt")), "-m", "20", "-q", "20", "-f", "0",
                                    "-F", "2316", "-d", "--where", where])
    assert (tmp_path / "device.txt").read_bytes() == (tmp_path / "host.txt").read_bytes()
    assert (tmp_path / "device.txt").read_text().count("\n") == len(loci_file_lines()) + 1


def test_a_damaged_block_sends_the_chunk_to_the_host_path(tmp_path):
    """one corrupted payload byte in a BGZF block that chrA's byte range holds and chrA's reads do not (it belongs to the next contig):
    the device path declines the chunk (inflate status or CRC-32), the host path - which never opens that block - gives the counts"""
    from clairs_to_amd._lib import check, lib
    c = case()
    raw = bytearray(open(c["bam"], "rb").read())
    offs, o = [], 0                                               # file offset of every BGZF block
    while o < len(raw):
        offs.append(o)
        o += struct.unpack_from("<H", raw, o + 16)[0] + 1
    header = 12 + sum(4 + len(n) + 1 + 4 for n, _ in REFS)
    first_7 = header + sum(len(_record(r, r["ref"])) for r in c["reads"] if r["ref"] == 0)       # where the other contig's records start
    k = first_7 // BLOCK_PAYLOAD + 2
    fb, fe = C.c_int64(), C.c_int64()
    check(lib.cto_bam_chunk_span(c["bam"].encode(), None, b"chrA", c["loci"]["chrA"][0], c["loci"]["chrA"][-1], C.byref(fb), C.byref(fe)))
    assert offs[k + 1] <= fe.value                                 # wholly inside what the device inflates for chrA
    raw[offs[k] + 18 + 7] ^= 0x5a
    bad = str(tmp_path / "bad.bam")
    open(bad, "wb").write(bytes(raw))
    shutil.copy(c["bam"] + ".bai", bad + ".bai")
    stats = {}
    got = _count("chrA", "verdict", "device", bam=bad, stats=stats)
    assert stats["fallback_chunks"] == 1 and stats["n_chunks"] == 1
    np.testing.assert_array_equal(got, expected("chrA", "verdict"))
    np.testing.assert_array_equal(got, _count("chrA", "verdict", "host", bam=bad))


@pytest.mark.parametrize("n_same", [600, 1500])
def test_many_reads_of_one_name(tmp_path, n_same):
    """a BAM whose names were stripped: 600 reads called `*` are linked on the device (every one is compared with the first that covers
    the locus), 1500 are more than the name table probes for, and the chunk goes to the host path - that is not a damaged chunk"""
    from clairs_to_amd.allele_counter import count_alleles
    rng = np.random.default_rng(n_same)
    reads = [dict(name="*", flag=0, ref=0, pos=int(p), mapq=60, cigar=[("M", 12), ("D", 1), ("M", 12)],
                  seq="".join(rng.choice(list("ACGT"), size=24)), qual=[30] * 24) for p in np.sort(rng.integers(0, 60, size=n_same))]
    reads.insert(5, dict(reads[5], name="other"))
    bam = str(tmp_path / "star.bam")
    write_bam(bam, [("c", 200)], reads, block_payload=BLOCK_PAYLOAD)
    loci = list(range(1, 100, 2))
    stats = {}
    got = count_alleles(bam, "c", loci, min_bq=20, min_mq=20, req_flags=0, excl_flags=2316, where="device", stats=stats)
    np.testing.assert_array_equal(got, naive_counts(reads, 0, loci, 20, 20, 0, 2316))
    np.testing.assert_array_equal(got, count_alleles(bam, "c", loci, min_bq=20, min_mq=20, req_flags=0, excl_flags=2316, where="host"))
    assert stats["fallback_chunks"] == 0 and stats["n_chunks"] == 1 and stats["n_reads_entered"] == n_same + 1


def test_many_tiny_blocks_grow_the_block_table(tmp_path):
    """64-byte BGZF payloads: the chunk holds more blocks than the first block table has entries (bytes / 2048 + 64), so the scan has
    to come back with a table eight times as large - the one loop the pipeline's device path shares"""
    from clairs_to_amd.allele_counter import count_alleles
    rng = np.random.default_rng(64)
    reads = [dict(name="r%03d" % i, flag=0, ref=0, pos=int(p), mapq=60, cigar=[("M", 10), ("I", 2), ("M", 12)],
                  seq="".join(rng.choice(list("ACGT"), size=24)), qual=[int(q) for q in rng.integers(10, 40, size=24)])
             for i, p in enumerate(np.sort(rng.integers(0, 370, size=300)))]
    bam = str(tmp_path / "tiny.bam")
    write_bam(bam, [("c", 400)], reads, block_payload=64)
    loci = list(range(3, 400, 8))
    stats = {}
    got = count_alleles(bam, "c", loci, min_bq=20, min_mq=20, req_flags=0, excl_flags=2316, where="device", stats=stats)
    np.testing.assert_array_equal(got, naive_counts(reads, 0, loci, 20, 20, 0, 2316))
    np.testing.assert_array_equal(got, count_alleles(bam, "c", loci, min_bq=20, min_mq=20, req_flags=0, excl_flags=2316, where="host"))
    assert stats["fallback_chunks"] == 0 and stats["n_chunks"] == 1
    assert stats["n_blocks"] > os.path.getsize(bam) // 2048 + 64           # the first table cannot have held them
