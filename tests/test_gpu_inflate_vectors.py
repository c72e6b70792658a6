"""csrc/inflate.hip on DEFLATE streams no encoder at hand writes (tests/deflate_catalogue.py: code lengths on both sides of the lookup
tables, every symbol's arithmetic, degenerate alphabets, code-length headers, block sequences, input-window boundaries at every payload
address modulo 4, match-queue fills, malformed streams) and on libdeflate's streams (tests/golden/libdeflate_blocks.json.gz).  Expected
bytes come from the token interpreter and zlib (tests/test_deflate_vectors.py), never from the kernel.  Every launch writes into a
buffer filled with a sentinel: a block may touch its own slot and CTO_BGZF_SLOT_PAD bytes behind its size, nothing else."""
import ctypes as C
import os
import re
import zlib

import numpy as np
import pytest

import deflate_catalogue as cat
import deflateutil as du
from test_deflate_vectors import load_libdeflate_blocks

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
FRONT = 256               # sentinel bytes in front of the first slot
with open(os.path.join(cat.ROOT, "include", "clairsto_amd.h")) as _f:
    SLOT_PAD = int(re.search(r"#define\s+CTO_BGZF_SLOT_PAD\s+(\d+)", _f.read()).group(1))


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def valid_vectors():
    return cat.valid_vectors()


@pytest.fixture(scope="module")
def neighbours():
    """ordinary zlib-made blocks that sit between the constructed ones: (block, data)"""
    rng = np.random.default_rng(21)
    texts = [bytes(rng.integers(33, 74, 3000, dtype=np.uint8)), (b"read%07d\t99\tchr1\t%d\t60\t100M\t=\t%d\t300\t" % (1, 2, 3)) * 60,
             bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 2500)), b"A", bytes(rng.integers(0, 256, 700, dtype=np.uint8))]
    out = []
    for i, t in enumerate(texts):
        co = zlib.compressobj((6, 1, 9, 6, 0)[i], zlib.DEFLATED, -15, 9)
        out.append((du.bgzf_data(co.compress(t) + co.flush(), t), t))
    return out


def inflate_into_sentinel(raw, dev):
    """bgzf.inflate_device with the output buffer filled with SENTINEL beforehand (FRONT bytes of it in front of the first slot):
    -> (block table, status array, output bytes with the guard in front)"""
    import torch
    from clairs_to_amd import bgzf
    from clairs_to_amd._lib import check, lib
    host = np.zeros(len(raw) + bgzf.BGZF_PAD, dtype=np.uint8)
    host[:len(raw)] = np.frombuffer(raw, dtype=np.uint8)
    tbl, out_bytes = bgzf.scan(host, len(raw))
    n = len(tbl)
    d_in = torch.from_numpy(host).to(dev)
    assert d_in.data_ptr() % 4 == 0                     # a payload's address modulo 4 is its in_off modulo 4
    d_blocks = torch.from_numpy(np.ascontiguousarray(tbl).view(np.uint8).reshape(-1)).to(dev)
    d_out = torch.full((FRONT + out_bytes,), SENTINEL, dtype=torch.uint8, device=dev)
    d_status = torch.full((n,), -1, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream(dev)
    check(lib.cto_bgzf_inflate(d_in.data_ptr(), d_blocks.data_ptr(), n, d_out.data_ptr() + FRONT, d_status.data_ptr(), C.c_void_p(s.cuda_stream)))
    torch.cuda.synchronize(dev)
    return tbl, d_status.cpu().numpy(), d_out.cpu().numpy()


def guard_failures(tbl, out, labels):
    """the sentinel in front of the first slot and from out_off + isize + SLOT_PAD to the next slot (the end of the buffer for the last)"""
    bad = []
    if not (out[:FRONT] == SENTINEL).all():
        bad.append("bytes in front of the first slot were written")
    for i in range(len(tbl)):
        lo = FRONT + int(tbl[i]["out_off"]) + int(tbl[i]["isize"]) + SLOT_PAD
        hi = FRONT + int(tbl[i + 1]["out_off"]) if i + 1 < len(tbl) else len(out)
        assert lo <= hi
        w = np.nonzero(out[lo:hi] != SENTINEL)[0]
        if len(w):
            bad.append("%s: byte %d behind its slot (isize + %d) was written" % (labels[i], int(w[0]), SLOT_PAD + int(w[0])))
    return bad


def exact_failure(tbl, st, out, i, label, want):
    """None, or what is wrong with block i: status, size, first differing byte"""
    if int(st[i]) != 0:
        from clairs_to_amd.bgzf import STATUS
        return "%s: status %d (%s)" % (label, int(st[i]), STATUS.get(int(st[i]), "?"))
    if int(tbl[i]["isize"]) != len(want):
        return "%s: ISIZE %d for %d bytes" % (label, int(tbl[i]["isize"]), len(want))
    o = FRONT + int(tbl[i]["out_off"])
    got = out[o:o + len(want)]
    ne = np.nonzero(got != np.frombuffer(want, dtype=np.uint8))[0]
    if len(ne):
        k = int(ne[0])
        return "%s: byte %d of %d is %d, not %d (%d bytes differ)" % (label, k, len(want), int(got[k]), want[k], len(ne))
    return None


def launch(entries, dev):
    """entries: (BGZF block, payload address modulo 4 or None, label, expected bytes or None) -> (rows, tbl, st, out, labels):
    rows[j] = the table row of entries[j]; fillers that move a payload to its address are checked here like any other valid block"""
    raw, order = du.place([(e[0], e[1]) for e in entries])
    tbl, st, out = inflate_into_sentinel(raw, dev)
    assert len(tbl) == len(order)
    rows, labels, failures = [], [], []
    for r, (kind, j, data) in enumerate(order):
        if kind == "filler":
            labels.append("filler in front of " + entries[j][2])
            failures.append(exact_failure(tbl, st, out, r, labels[-1], data))
        else:
            labels.append(entries[j][2])
            rows.append(r)
            if entries[j][1] is not None:
                assert int(tbl[r]["in_off"]) % 4 == entries[j][1]
            if entries[j][3] is not None:
                failures.append(exact_failure(tbl, st, out, r, labels[-1], entries[j][3]))
    failures = [f for f in failures if f] + guard_failures(tbl, out, labels)
    return rows, tbl, st, out, failures


@pytest.mark.parametrize("turn", [0, 1, 2, 3])
def test_valid_vectors(dev, valid_vectors, neighbours, turn):
    """every valid vector in one launch, vector i at payload address (i + turn) modulo 4 - over the four launches each vector sits at all
    four -, a zlib-made block after every eighth: status 0, zlib's bytes, sentinel intact"""
    entries = []
    for i, v in enumerate(valid_vectors):
        r = (i + turn) % 4
        entries.append((du.bgzf_wrap(v.payload, v.isize, v.crc), r, "%s [address %d mod 4]" % (v.name, r), v.expected))
        if i % 8 == 0:
            blk, data = neighbours[(i // 8) % len(neighbours)]
            entries.append((blk, None, "zlib-made neighbour behind " + v.name, data))
    _, _, _, _, failures = launch(entries, dev)
    assert not failures, "%d failures:\n%s" % (len(failures), "\n".join(failures[:40]))


def test_isize_65536(dev, valid_vectors):
    """a block of 65536 bytes - one more than BSIZE lets a writer store, but what ISIZE can claim: cto_bgzf_scan takes it and the device
    decodes it exactly (a queue entry's 16-bit destination and source fields hold every position below 65536)"""
    from clairs_to_amd.bgzf import inflate_bytes
    v = [x for x in valid_vectors if x.isize == 65536]
    assert len(v) == 1 and len(v[0].payload) < 1000
    got = inflate_bytes(du.bgzf_wrap(v[0].payload, v[0].isize, v[0].crc), dev)
    assert got == [v[0].expected]


def test_malformed_vectors(dev, neighbours):
    """each malformed stream at all four payload addresses between intact zlib-made blocks, one launch: the status the stream's path
    must end with (any non-zero one where more than one is possible; status or CRC-32 for the two incomplete sets the kernel does not
    refuse at the table), intact neighbours, sentinel intact"""
    vectors = cat.malformed_vectors()
    entries = [(neighbours[0][0], None, "zlib-made block in front", neighbours[0][1])]
    for i, v in enumerate(vectors):
        for r in range(4):
            entries.append((du.bgzf_wrap(v.payload, v.isize, v.crc), r, "%s [address %d mod 4]" % (v.name, r), None))
            blk, data = neighbours[(4 * i + r + 1) % len(neighbours)]
            entries.append((blk, None, "zlib-made block behind " + v.name, data))
    rows, tbl, st, out, failures = launch(entries, dev)
    k = 0
    for j, e in enumerate(entries):
        if e[3] is not None:
            continue
        v, r = vectors[(j - 1) // 8], rows[j]
        status = int(st[r])
        if v.weak:
            o = FRONT + int(tbl[r]["out_off"])
            if status == 0 and zlib.crc32(out[o:o + v.isize].tobytes()) == v.crc:
                failures.append("%s: status 0 and the trailer's CRC-32" % e[2])
        elif v.status is None:
            if status == 0:
                failures.append("%s: status 0" % e[2])
        elif status != v.status:
            failures.append("%s: status %d, not %d" % (e[2], status, v.status))
        k += 1
    assert k == 4 * len(vectors)
    assert not failures, "%d failures:\n%s" % (len(failures), "\n".join(failures[:40]))


def test_libdeflate_streams(dev):
    """the committed libdeflate streams (levels 1, 6, 12) wrapped as BGZF blocks, each at all four payload addresses, one launch"""
    entries = []
    for i, (label, stream, data) in enumerate(load_libdeflate_blocks()):
        for r in range(4):
            entries.append((du.bgzf_data(stream, data), r, "libdeflate %s [address %d mod 4]" % (label, r), data))
    _, _, _, _, failures = launch(entries, dev)
    assert not failures, "%d failures:\n%s" % (len(failures), "\n".join(failures[:40]))
