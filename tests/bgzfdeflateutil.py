"""Inputs and checks shared by tests/test_bgzf_deflate.py (host restatement) and tests/test_gpu_bgzf_deflate.py (device == host):
the shapes the BGZF coder (csrc/deflate.hip, csrc/deflate_host.h) is held to, a decoder of DEFLATE tokens, and the crafted block whose
parse uses every match length and both edges of every distance code."""
import ctypes as C
import struct
import zlib

import numpy as np

PAYLOAD = 0xff00
SEG = 512                      # csrc/deflate_host.h: CTO_DEFLATE_SEG
PROBES = (1, 2, 3, 4, 6, 8)    # CTO_DEFLATE_PROBES
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
# both edges of every distance code
DIST_EDGES = [1, 2, 3, 4] + [e for k in range(1, 14) for lo in ((1 << (k + 1)) + 1, (1 << (k + 1)) + (1 << k) + 1) for e in (lo, lo + (1 << k) - 1)]
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in (0, 1)]


def rng_bytes(n, seed, lo=0, hi=256):
    return np.random.RandomState(seed).randint(lo, hi, size=n).astype(np.uint8).tobytes()


def bam_like(n, seed):
    """low-entropy bytes with runs, as qualities and packed bases have them"""
    r = np.random.RandomState(seed)
    out = bytearray()
    while len(out) < n:
        out += bytes([int(r.choice([17, 33, 34, 65, 66, 72, 129, 136]))]) * int(r.randint(1, 9))
        if r.randint(0, 6) == 0:
            out += out[-int(r.randint(20, 400)):][:int(r.randint(4, 60))]
    return bytes(out[:n])


def shapes():
    """name -> input bytes"""
    s = {"n%d" % n: bam_like(n, n) for n in (0, 1, 2, 3, 4)}
    s["payload-1"] = bam_like(PAYLOAD - 1, 11)
    s["payload"] = bam_like(PAYLOAD, 12)
    s["payload+1"] = bam_like(PAYLOAD + 1, 13)
    s["2payload+7"] = bam_like(2 * PAYLOAD + 7, 14)
    s["equal"] = b"I" * PAYLOAD
    s["period2"] = b"ab" * (PAYLOAD // 2)
    s["period3"] = b"abc" * (PAYLOAD // 3)
    s["random"] = rng_bytes(PAYLOAD, 15)
    s["all_bytes"] = bytes(range(256)) * 3 + b"".join(bytes([b]) * (1 + b % 5) + b"the quick brown fox " for b in range(256))
    s["crafted"] = crafted_block()
    far = bytearray(rng_bytes(32769 + 80, 16))
    far[32769:] = far[:80]                                # the only repeat lies 32769 back
    s["far"] = bytes(far)
    seg = bytearray(rng_bytes(3 * SEG, 17))
    seg[SEG - 10:SEG + 30] = seg[100:140]                 # a repeat of 40 bytes that starts 10 bytes before a segment's end
    seg[3 * SEG - 50:] = seg[900:950]                     # and one that runs to the block's end
    s["segment_end"] = bytes(seg)
    s["no_match"] = de_bruijn(b"ACGT!I", 3)               # every three of six bytes once: nothing to copy, much to gain from a code
    return s


def de_bruijn(alphabet, n):
    """the de Bruijn sequence B(k, n), not wrapped around: len(alphabet) ** n bytes in which no run of n bytes comes twice"""
    k, a, seq = len(alphabet), [0] * (len(alphabet) * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return bytes(alphabet[i] for i in seq)


def hash4(b, p):
    return ((struct.unpack_from("<I", b, p)[0] * 2654435761) & 0xffffffff) >> 18


class Table(object):
    """the hash table of rule 3 over a buffer that only grows: candidate(p) = the largest q below p's tile with p's hash"""

    def __init__(self, b):
        self.b, self.last, self.upto = b, {}, 0

    def candidate(self, p):
        b, t0 = self.b, p // 256 * 256
        while self.upto < t0 - 3:                          # these four bytes lie below the tile: they no longer change
            self.last[hash4(b, self.upto)] = self.upto
            self.upto += 1
        h = hash4(b, p)
        best = self.last.get(h, -1)
        for q in range(max(0, t0 - 3), t0):
            if q + 4 <= len(b) and hash4(b, q) == h:
                best = q
        return best


def match_at(b, n, p, table=None):
    """rule 3 of csrc/deflate.hip restated: (length, distance) or None"""
    seg_end = min(n, (p // SEG + 1) * SEG)
    max_len = min(258, seg_end - p)
    if max_len < 3:
        return None
    cands = [p - d for d in PROBES]
    if p + 4 <= n:
        cands.append((table or Table(b)).candidate(p))
    best = None
    for q in cands:
        if q < 0 or p - q > 32768:
            continue
        ln = 0
        while ln < max_len and b[q + ln] == b[p + ln]:
            ln += 1
        if best is None or ln > best[0] or (ln == best[0] and p - q < best[1]):
            best = (ln, p - q)
    if best is None or best[0] < 3 or (best[0] == 3 and best[1] > 4096):
        return None
    return best


_CRAFTED = []


def crafted_block():
    """One block in which a copy of every length 3 .. 258 is found, at distances that are the two edges of every distance code.  Units
    are laid one after the other behind random bytes: [B, B + L) = a copy of [B - D, B - D + L), then a byte that ends the match; a
    unit is moved on by one random byte until match_at (above) finds exactly (L, D) at B.  Distances below 256 are seen by the hash
    table only from the first positions of a tile, the distances 1, 2, 3, 4, 6, 8 by the probes anywhere.
    The walk of the segment must arrive at B, so the bytes in front of a unit may not hold a match that reaches over it."""
    if _CRAFTED:
        return _CRAFTED[0]
    r = np.random.RandomState(99)
    b = bytearray(rng_bytes(20000, 98))
    lens = list(range(3, 259))
    far = [d for d in DIST_EDGES if d > 256]
    near = [d for d in DIST_EDGES if d <= 256 and d not in PROBES]
    stale = []                 # what has been a source: its bytes lie once more further on, and the table names the later place
    table = Table(b)
    walk = [0]                 # where the greedy walk stands: everything before it is decided

    def lay(ln, d):
        """the unit (ln, d) at the end of b if it can stand there and is found as such"""
        B = len(b)
        s_left = SEG - B % SEG
        if not (s_left >= ln and B - d >= 0 and (d in PROBES or d > B % 256) and B + ln + 1 <= PAYLOAD - 8):
            return False
        if any(lo < B - d + ln + 4 and B - d < hi for lo, hi in stale):
            return False
        for i in range(ln):
            b.append(b[B - d + i])
        b.append(b[B - d + ln] ^ 0x55 if s_left > ln and ln < 258 else int(r.randint(0, 256)))
        p = max(walk[0], B // SEG * SEG)
        while p < B:                                       # the walk has to come by B: no match on the way may reach over it
            m = match_at(b, len(b), p, table)
            p += m[0] if m else 1
        if p == B and match_at(b, len(b), B, table) == (ln, d):
            stale.append((B - d, B - d + ln))
            walk[0] = B + ln
            return True
        del b[B:]
        return False

    # the probes and the near distances first, with the short lengths (length 3 needs a distance of at most 4096)
    for d in list(PROBES) + near:
        ln = lens.pop(0)
        while not lay(ln, d):
            b.append(int(r.randint(0, 256)))
    need = list(far)
    for ln in lens:
        while True:
            tried = 0
            for d in need + far:
                if tried == 4:
                    continue
                if d <= len(b) and not any(lo < len(b) - d + ln + 4 and len(b) - d < hi for lo, hi in stale):
                    tried += 1
                    if lay(ln, d):
                        break
            else:
                b.append(int(r.randint(0, 256)))
                assert len(b) < PAYLOAD - 300, "the crafted block does not fit: adjust the generator"
                continue
            if d in need:
                need.remove(d)
            break
    assert not need, "distances left over: adjust the generator"
    b += rng_bytes(8, 97)
    _CRAFTED.append(bytes(b))
    return _CRAFTED[0]


class Bits(object):
    def __init__(self, data):
        self.d, self.pos = data, 0

    def take(self, n):
        v = 0
        for i in range(n):
            v |= ((self.d[self.pos >> 3] >> (self.pos & 7)) & 1) << i
            self.pos += 1
        return v


def _decoder(lengths):
    """canonical Huffman code -> {(length, code): symbol}"""
    count, code, nxt = [0] * 16, 0, [0] * 16
    for ln in lengths:
        count[ln] += 1
    count[0] = 0
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    table = {}
    for sym, ln in enumerate(lengths):
        if ln:
            table[ln, nxt[ln]] = sym
            nxt[ln] += 1
    return table


def _symbol(bits, table):
    code = 0
    for ln in range(1, 16):
        code = (code << 1) | bits.take(1)
        if (ln, code) in table:
            return table[ln, code]
    raise ValueError("no such code")


def tokens(payload):
    """the tokens of a one-block DEFLATE stream: (block type, [(0, byte) | (length, distance)], code lengths or None)"""
    bits = Bits(payload)
    assert bits.take(1) == 1
    kind = bits.take(2)
    if kind == 0:
        return 0, [], None
    if kind == 1:
        ll, dd = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, [5] * 30
    else:
        hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
        cl = [0] * 19
        for k in range(hclen):
            cl[(16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)[k]] = bits.take(3)
        clt, seq = _decoder(cl), []
        while len(seq) < hlit + hdist:
            s = _symbol(bits, clt)
            if s < 16:
                seq.append(s)
            elif s == 16:
                seq += [seq[-1]] * (3 + bits.take(2))
            else:
                seq += [0] * ((3 + bits.take(3)) if s == 17 else (11 + bits.take(7)))
        assert len(seq) == hlit + hdist
        ll, dd = seq[:hlit], seq[hlit:]
    llt, ddt, out = _decoder(ll), _decoder(dd), []
    while True:
        s = _symbol(bits, llt)
        if s == 256:
            break
        if s < 256:
            out.append((0, s))
            continue
        ln = LEN_BASE[s - 257] + bits.take(LEN_EXTRA[s - 257])
        ds = _symbol(bits, ddt)
        out.append((ln, DIST_BASE[ds] + bits.take(DIST_EXTRA[ds])))
    assert (bits.pos + 7) // 8 == len(payload)
    return kind, out, (ll, dd)


def split_blocks(raw):
    """[(payload, crc, isize, whole size)] of a run of BGZF blocks"""
    out, o = [], 0
    while o < len(raw):
        assert raw[o:o + 4] == b"\x1f\x8b\x08\x04" and raw[o + 10:o + 16] == b"\x06\x00BC\x02\x00"
        bsize = struct.unpack_from("<H", raw, o + 16)[0] + 1
        crc, isize = struct.unpack_from("<II", raw, o + bsize - 8)
        out.append((raw[o + 18:o + bsize - 8], crc, isize, bsize))
        o += bsize
    assert o == len(raw)
    return out


def check_blocks(raw, blocks_bytes, sizes):
    """the round trip of one input: inflated bytes, CRC-32, ISIZE, BSIZE and the size bound of every block"""
    blocks = split_blocks(blocks_bytes)
    assert len(blocks) == len(sizes) == (len(raw) + PAYLOAD - 1) // PAYLOAD
    for k, (payload, crc, isize, bsize) in enumerate(blocks):
        want = raw[k * PAYLOAD:(k + 1) * PAYLOAD]
        d = zlib.decompressobj(-15)
        assert d.decompress(payload) + d.flush() == want and d.eof and not d.unused_data
        assert crc == zlib.crc32(want) & 0xffffffff and isize == len(want)
        assert bsize == int(sizes[k]) <= len(want) + 31


def block_sizes(block, where):
    from clairs_to_amd._lib import check, lib
    buf = np.frombuffer(block, dtype=np.uint8) if len(block) else np.zeros(1, np.uint8)
    bits, hist = np.zeros(3, dtype=np.int64), np.zeros(316, dtype=np.uint32)
    check(lib.cto_deflate_block_sizes(buf.ctypes.data, len(block), {"device": 0, "host": 1}[where], bits.ctypes.data, hist.ctypes.data))
    return [int(x) for x in bits], hist


def code_lengths(freq, max_bits, where):
    from clairs_to_amd._lib import check, lib
    f = np.ascontiguousarray(freq, dtype=np.uint32)
    out = np.zeros(len(f), dtype=np.uint8)
    check(lib.cto_deflate_code_lengths(f.ctypes.data, len(f), int(max_bits), {"device": 0, "host": 1}[where], out.ctypes.data))
    return [int(x) for x in out]


def fibonacci_freq(n_used, n_sym, stride=1):
    """Fibonacci frequencies on n_used of n_sym symbols: the Huffman tree of such weights is a chain, n_used - 1 deep"""
    f, a, b = [0] * n_sym, 1, 1
    for k in range(n_used):
        f[(k * stride) % n_sym] = a
        a, b = b, a + b
    return f
