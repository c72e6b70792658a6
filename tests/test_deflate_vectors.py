"""The hand-assembled DEFLATE streams of tests/deflate_catalogue.py against zlib (and libdeflate where it loads): the reference has to
agree with the token interpreter on every valid vector and refuse every malformed one before the device is asked
(tests/test_gpu_inflate_vectors.py).  The catalogue's own coverage assertions - code widths, window boundaries, queue fills - run while
it is built, here as there."""
import base64
import ctypes
import ctypes.util
import hashlib
import time
import zlib

import numpy as np
import pytest

import deflate_catalogue as cat
import deflateutil as du


@pytest.fixture(scope="module")
def valid_vectors():
    return cat.valid_vectors()


@pytest.fixture(scope="module")
def malformed_vectors():
    return cat.malformed_vectors()


def load_libdeflate_blocks():
    """the fixture of tests/golden/gen_libdeflate_blocks.py with its payloads regenerated from their seeds and checked against the stored
    SHA-256 (a drifting generator fails here, not as a decoder mismatch): list of (label, raw DEFLATE stream, payload)"""
    from conftest import load_json_gz
    import gen_libdeflate_blocks as gen
    g = load_json_gz("libdeflate_blocks.json.gz")
    data = dict(((kind, seed), d) for kind, seed, _, d in gen.payloads())
    out = []
    for b in g["blocks"]:
        d = data[(b["kind"], b["seed"])]
        assert len(d) == b["n"] and hashlib.sha256(d).hexdigest() == b["sha256"], (b["kind"], b["seed"])
        out.append(("%s seed %d level %d" % (b["kind"], b["seed"], b["level"]), base64.b64decode(b["deflate_b64"]), d))
    assert len(out) == len(gen.SPECS) * len(gen.LEVELS)
    return out


def test_writer_is_fast_and_exact():
    """a 64 KiB stream assembles in well under a second; canonical codes and the Kraft sum as RFC 1951 3.2.2 has them"""
    assert du.canonical([3, 3, 3, 3, 3, 2, 4, 4]) == [2, 3, 4, 5, 6, 0, 14, 15]          # the RFC's own example
    assert du.kraft([3, 3, 3, 3, 3, 2, 4, 4]) == 1 and du.kraft([1, 1, 1]) > 1 and du.kraft([1, 0, 2]) < 1
    data = bytes(np.random.default_rng(0).integers(0, 256, 65536, dtype=np.uint8))
    t0 = time.perf_counter()
    s = du.Stream().fixed([("lit", x) for x in data], final=True)
    p = s.payload()
    dt = time.perf_counter() - t0
    assert du.inflate_zlib(p) == (data, True, b"") and bytes(s.out) == data
    assert dt < 1.0, "assembling 65536 literals took %.2f s" % dt
    k, off, w = s.w.log()
    assert k[0] == du.HDR and off[1] == 3 and int(off[-1] + w[-1]) == s.nbits and len(p) == (s.nbits + 7) // 8


def test_placement_gives_every_residue():
    blk = du.bgzf_data(du.Stream().fixed([("lit", 65)], final=True).payload(), b"A")
    raw, order = du.place([(blk, r) for r in (0, 1, 2, 3, 3, 1, 0, 2)])
    o, seen = 0, []
    for kind, _, _ in order:
        bsize = int.from_bytes(raw[o + 16:o + 18], "little") + 1
        if kind == "block":
            seen.append((o + 18) % 4)
        o += bsize
    assert o == len(raw) and seen == [0, 1, 2, 3, 3, 1, 0, 2]


def test_valid_vectors_decode_under_zlib(valid_vectors):
    assert len(valid_vectors) > 200
    for v in valid_vectors:
        out, eof, unused = du.inflate_zlib(v.payload)
        assert eof and unused == b"", v.name
        assert out == v.expected, "%s: zlib and the token interpreter differ" % v.name
        assert v.zlib_says == "ok" and v.status == 0 and v.isize == len(out) and v.crc == zlib.crc32(out)
        assert len(v.payload) + 26 <= 65536, v.name


def test_valid_vectors_decode_under_libdeflate(valid_vectors):
    """a second, unrelated decoder; without the library only this extra check is void"""
    name = ctypes.util.find_library("deflate") or "libdeflate.so.0"
    try:
        ld = ctypes.CDLL(name)
    except OSError:
        return
    ld.libdeflate_alloc_decompressor.restype = ctypes.c_void_p
    ld.libdeflate_deflate_decompress.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                                                 ctypes.POINTER(ctypes.c_size_t)]
    ld.libdeflate_free_decompressor.argtypes = [ctypes.c_void_p]
    d = ld.libdeflate_alloc_decompressor()
    try:
        for v in valid_vectors:
            buf = ctypes.create_string_buffer(len(v.expected))
            n = ctypes.c_size_t(0)
            rc = ld.libdeflate_deflate_decompress(d, v.payload, len(v.payload), buf, len(v.expected), ctypes.byref(n))
            assert rc == 0 and n.value == len(v.expected) and buf.raw == v.expected, "%s: libdeflate returns %d" % (v.name, rc)
    finally:
        ld.libdeflate_free_decompressor(d)


def test_malformed_vectors_are_refused_by_zlib(malformed_vectors):
    assert len(malformed_vectors) == 16
    for v in malformed_vectors:
        assert v.expected is None and v.zlib_says != "ok"
        try:
            out, eof, _ = du.inflate_zlib(v.payload)
        except zlib.error:
            assert v.zlib_says == "error", v.name
            continue
        assert v.zlib_says != "error", v.name
        assert not eof or len(out) != v.isize or zlib.crc32(out) != v.crc, "%s decodes to what its trailer claims" % v.name
        assert (v.zlib_says == "truncated") == (not eof), v.name
        if eof:
            assert (v.zlib_says == "long") == (len(out) > v.isize) and (v.zlib_says == "short") == (len(out) < v.isize), v.name


def test_catalogue_coverage(valid_vectors):
    """what groups A, F and G promise, from the event logs: code widths on both sides of the kernel's table sizes, an input-window
    boundary inside every kind of item at every payload address modulo 4, queue fills around the kernel's TOK"""
    w_ll, w_d, n_match = set(), set(), set()
    for v in valid_vectors:
        w_ll |= cat.widths(v.log, du.LIT) | cat.widths(v.log, du.LEN) | cat.widths(v.log, du.EOB)
        w_d |= cat.widths(v.log, du.DIST)
        if v.name.startswith("G/") and int((v.log[0] == du.HDR).sum()) == 1:
            n_match.add(cat.n_matches(v.log))
    assert w_ll == set(range(1, 16)) and w_d == set(range(1, 16))
    for kind in (du.LIT, du.LEN, du.EOB):
        got = set().union(*(cat.widths(v.log, kind) for v in valid_vectors))
        assert {cat.TBL, cat.TBL + 1, 15} <= got, (du.KIND_NAMES[kind], sorted(got))
    assert {cat.TBD, cat.TBD + 1, 15} <= w_d
    assert {cat.TOK - 1, cat.TOK, cat.TOK + 1} <= n_match and max(n_match) >= 300
    for r in range(4):
        hit = set()
        for v in valid_vectors:
            hit |= cat.window_hits(v.log, r)
        assert hit >= set(cat.F_KINDS), "payload address %d mod 4: no window boundary in %r" % (r, set(cat.F_KINDS) - hit)
    sizes = set(v.isize for v in valid_vectors)
    assert {1, 65280, 65536} <= sizes


def test_libdeflate_fixture_decodes_under_zlib():
    blocks = load_libdeflate_blocks()
    kinds = set()
    for label, stream, data in blocks:
        assert du.inflate_zlib(stream) == (data, True, b""), label
        kinds.add(stream[0] >> 1 & 3)
    assert 2 in kinds              # dynamic first blocks (stored ones where the payload is incompressible)
