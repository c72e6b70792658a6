"""Writes libdeflate_blocks.json.gz: raw DEFLATE streams of seeded payloads as libdeflate writes them - the encoder behind htslib, and
so behind most BAM files - at levels 1, 6 and 12.  libdeflate splits blocks and shapes codes unlike zlib (tests/test_gpu_inflate.py's only
encoder).  The fixture stores each payload's kind, seed and SHA-256; the tests regenerate the payloads from payloads() below and read the
streams from the fixture, so they need no libdeflate.

    python tests/golden/gen_libdeflate_blocks.py        (needs libdeflate.so.0)
"""
import base64
import ctypes
import gzip
import hashlib
import json
import os

import numpy as np

LEVELS = (1, 6, 12)
SPECS = [("records", 1, 20000), ("records", 2, 9000), ("records", 3, 700), ("quals", 4, 20000), ("quals", 5, 5000), ("acgt", 6, 20000),
         ("acgt", 7, 3000), ("period", 8, 20000), ("period", 9, 4097), ("random", 10, 6000), ("random", 11, 300), ("mixed", 12, 20000)]


def make_payload(kind, seed, n):
    rng = np.random.default_rng(seed)
    if kind == "records":                    # BAM-record-like text: names that count up, repeated fields, a sequence and its qualities
        rows, pos = [], int(rng.integers(10000, 90000))
        for i in range(n // 60 + 2):
            pos += int(rng.integers(1, 40))
            seq = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 36))
            qual = bytes(rng.integers(33, 74, 36, dtype=np.uint8))
            rows.append(b"read%07d\t%d\tchr1\t%d\t60\t36M\t=\t%d\t%d\t%s\t%s\n" % (seed * 100000 + i, 99 if i % 2 else 147, pos, pos + 300, 336, seq, qual))
        return b"".join(rows)[:n]
    if kind == "quals":
        return bytes(rng.integers(33, 74, n, dtype=np.uint8))
    if kind == "acgt":
        return bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n))
    if kind == "period":
        p = bytes(rng.integers(0, 256, int(rng.integers(2, 9)), dtype=np.uint8))
        return (p * (n // len(p) + 1))[:n]
    if kind == "random":
        return bytes(rng.integers(0, 256, n, dtype=np.uint8))
    if kind == "mixed":
        parts = [make_payload(k, seed * 31 + j, n // 4) for j, k in enumerate(("records", "random", "period", "quals"))]
        return b"".join(parts)[:n]
    raise ValueError(kind)


def payloads():
    return [(kind, seed, n, make_payload(kind, seed, n)) for kind, seed, n in SPECS]


def main():
    ld = ctypes.CDLL("libdeflate.so.0")
    ld.libdeflate_alloc_compressor.restype = ctypes.c_void_p
    ld.libdeflate_alloc_compressor.argtypes = [ctypes.c_int]
    ld.libdeflate_deflate_compress.restype = ctypes.c_size_t
    ld.libdeflate_deflate_compress.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
    ld.libdeflate_free_compressor.argtypes = [ctypes.c_void_p]
    blocks = []
    for kind, seed, n, data in payloads():
        assert len(data) == n <= 20000
        for level in LEVELS:
            c = ld.libdeflate_alloc_compressor(level)
            buf = ctypes.create_string_buffer(2 * n + 1024)
            got = ld.libdeflate_deflate_compress(c, data, n, buf, len(buf))
            ld.libdeflate_free_compressor(c)
            assert got > 0
            blocks.append(dict(kind=kind, seed=seed, n=n, level=level, sha256=hashlib.sha256(data).hexdigest(),
                               deflate_b64=base64.b64encode(buf.raw[:got]).decode()))
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libdeflate_blocks.json.gz")
    with gzip.GzipFile(out, "wb", mtime=0) as f:
        f.write(json.dumps(dict(encoder="libdeflate_deflate_compress", levels=list(LEVELS), blocks=blocks), sort_keys=True).encode())
    print(out, os.path.getsize(out), "bytes,", len(blocks), "streams")


if __name__ == "__main__":
    main()
