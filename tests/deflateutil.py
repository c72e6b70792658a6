"""A DEFLATE (RFC 1951) / BGZF writer for tests: streams are assembled item by item - block headers, code-length symbols, literal, length
and distance codes, extra bits, stored bytes - so that a test decides which path of a decoder runs instead of leaving it to an encoder.
Every emitted item is logged with its bit offset; an interpreter turns the same token list into the bytes the stream stands for."""
import struct
import zlib
from fractions import Fraction

import numpy as np

# item kinds of the event log
HDR, COUNTS, CL_TRIPLE, CL_SYM, CL_EXTRA, LIT, LEN, LEN_EXTRA, DIST, DIST_EXTRA, EOB, PAD, LEN_NLEN, STORED = range(14)
KIND_NAMES = ["block header", "HLIT/HDIST/HCLEN", "code-length triple", "code-length symbol", "code-length repeat bits", "literal code",
              "length code", "length extra bits", "distance code", "distance extra bits", "end-of-block code", "byte alignment",
              "LEN/NLEN", "stored byte"]

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
         16385, 24577]
DEXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


def kraft(lens):
    """sum of 2^-len over the non-zero lengths: 1 for a complete code, more for an over-subscribed one"""
    return sum((Fraction(1, 1 << l) for l in lens if l), Fraction(0))


def canonical(lens):
    """RFC 1951 3.2.2: code of every symbol (None where the length is 0), MSB first"""
    bl_count = [0] * 17
    for l in lens:
        bl_count[l] += 1
    bl_count[0] = 0
    next_code = [0] * 17
    code = 0
    for bits in range(1, 17):
        code = (code + bl_count[bits - 1]) << 1
        next_code[bits] = code
    out = []
    for l in lens:
        if l:
            out.append(next_code[l])
            next_code[l] += 1
        else:
            out.append(None)
    return out


def _rev(code, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (code & 1)
        code >>= 1
    return r


def _revcodes(lens):
    """(code in stream bit order, length) per symbol; over-subscribed sets still get (overflowing, truncated) codes"""
    return [(_rev(c & ((1 << l) - 1), l), l) if l else (0, 0) for c, l in zip(canonical(lens), lens)]


def complete_lengths(n):
    """lengths of a complete code over n >= 2 symbols, as even as possible, ascending"""
    assert n >= 2
    k = n.bit_length() - 1
    return [k] * ((2 << k) - n) + [k + 1] * (2 * (n - (1 << k)))


def staircase(n):
    """1, 2, ..., n-1, n-1: the complete code with the widest spread of lengths over n symbols"""
    return list(range(1, n)) + [n - 1]


def stair_plus(n_short, n_long):
    """n_short symbols on 1..n_short bits, the remaining 2^-n_short shared evenly by n_long symbols: (short lengths, long lengths)"""
    longs = [n_short + l for l in complete_lengths(n_long)]
    assert max(longs) <= 15
    return list(range(1, n_short + 1)), longs


def assign(n, pairs):
    """code-length list of n symbols from (symbol, length) pairs"""
    lens = [0] * n
    for s, l in pairs:
        assert lens[s] == 0
        lens[s] = l
    return lens


def length_symbol(length):
    assert 3 <= length <= 258
    if length == 258:
        return 285, 0
    ls = max(i for i in range(28) if LBASE[i] <= length)
    return 257 + ls, length - LBASE[ls]


def dist_symbol(dist):
    assert 1 <= dist <= 32768
    ds = max(i for i in range(30) if DBASE[i] <= dist)
    return ds, dist - DBASE[ds]


def as_raw(t):
    if t[0] == "match":
        ls, lx = length_symbol(t[1])
        ds, dx = dist_symbol(t[2])
        return ("raw", ls, lx, ds, dx)
    return t


def interpret(tokens, out=None):
    """the bytes a token list stands for, appended to `out` (what earlier blocks produced); stops at ("eob",)"""
    out = bytearray() if out is None else out
    for t in tokens:
        t = as_raw(t)
        if t[0] == "lit":
            out.append(t[1])
        elif t[0] == "eob":
            break
        elif t[0] == "bits":
            raise ValueError("free-form bits have no meaning")
        else:
            _, ls, lx, ds, dx = t
            if ds is None or not (257 <= ls <= 285 and 0 <= ds <= 29):
                raise ValueError("reserved symbol")
            n, d = LBASE[ls - 257] + lx, DBASE[ds] + dx
            if d > len(out):
                raise ValueError("distance %d beyond the %d bytes so far" % (d, len(out)))
            for _ in range(n):
                out.append(out[-d])
    return out


def plain_cl_seq(lens):
    return [(l,) for l in lens]


def rle_cl_seq(lens, allowed=(16, 17, 18)):
    """greedy run-length coding of a code-length list with the repeat symbols in `allowed`"""
    seq, i, n = [], 0, len(lens)
    while i < n:
        v = lens[i]
        run = 1
        while i + run < n and lens[i + run] == v:
            run += 1
        if v == 0 and run >= 11 and 18 in allowed:
            r = min(run, 138)
            seq.append((18, r))
        elif v == 0 and run >= 3 and 17 in allowed:
            r = min(run, 10)
            seq.append((17, r))
        elif v != 0 and run >= 4 and 16 in allowed:
            seq.append((v,))
            r = min(run - 1, 6)
            seq.append((16, r))
            r += 1
        else:
            seq.append((v,))
            r = 1
        i += r
    return seq


def expand_cl_seq(seq):
    out = []
    for e in seq:
        if e[0] < 16:
            out.append(e[0])
        elif e[0] == 16:
            out.extend([out[-1]] * e[1])
        else:
            out.extend([0] * e[1])
    return out


class BitWriter(object):
    """LSB-first fields, Huffman codes MSB first; remembers kind, bit offset and width of every item"""

    def __init__(self):
        self.vals, self.widths, self.kinds = [], [], []
        self.nbits = 0

    def put(self, val, n, kind):
        assert 0 <= val < (1 << n) or n == 0
        if n:
            self.vals.append(val)
            self.widths.append(n)
            self.kinds.append(kind)
            self.nbits += n

    def code(self, code, n, kind):
        self.put(_rev(code, n), n, kind)

    def align(self):
        self.put(0, -self.nbits % 8, PAD)

    def put_bytes(self, data, kind):
        self.vals.extend(data)
        self.widths.extend([8] * len(data))
        self.kinds.extend([kind] * len(data))
        self.nbits += 8 * len(data)

    def log(self):
        """(kind, bit offset, width) arrays, one entry per item"""
        w = np.asarray(self.widths, dtype=np.int64)
        return np.asarray(self.kinds, dtype=np.int64), np.cumsum(w) - w, w

    def getvalue(self):
        if not self.vals:
            return b""
        w = np.asarray(self.widths, dtype=np.int64)
        v = np.asarray(self.vals, dtype=np.uint64)
        off = np.cumsum(w) - w
        total = int(w.sum())
        pos = np.arange(total, dtype=np.int64) - np.repeat(off, w)
        bits = ((np.repeat(v, w) >> pos.astype(np.uint64)) & np.uint64(1)).astype(np.uint8)
        return np.packbits(bits, bitorder="little").tobytes()


class Stream(object):
    """one DEFLATE stream: block emitters over a BitWriter plus the bytes the blocks stand for (self.out; None once a block
    is emitted that has no meaning)"""

    def __init__(self):
        self.w = BitWriter()
        self.out = bytearray()

    # -- blocks -------------------------------------------------------------------------------------------------------------
    def header(self, final, btype):
        self.w.put(int(bool(final)) | (btype << 1), 3, HDR)

    def stored(self, data, final=False, nlen=None):
        data = bytes(data)
        assert len(data) <= 65535
        self.header(final, 0)
        self.w.align()
        self.w.put(len(data), 16, LEN_NLEN)
        self.w.put((len(data) ^ 0xffff) if nlen is None else nlen, 16, LEN_NLEN)
        self.w.put_bytes(data, STORED)
        if self.out is not None:
            self.out += data
        return self

    def fixed(self, tokens, final=False, eob=True):
        self.header(final, 1)
        self._tokens(tokens, _FIXED_LL_CODES, _FIXED_D_CODES, eob)
        return self

    def dynamic(self, tokens, ll_lens, d_lens, final=False, eob=True, cl_seq=None, cl_lens=None, hclen=None, check=True):
        """ll_lens: 257..286 literal / length code lengths, d_lens: 1..30 distance code lengths, cl_seq: how the two lists are
        written - (length,), (16, repeats), (17, repeats), (18, repeats) -, cl_lens: lengths of the 19 code-length codes,
        hclen: how many of them are written.  check=False lets a malformed header through."""
        if cl_seq is None:
            cl_seq = rle_cl_seq(list(ll_lens) + list(d_lens))
        if check:
            assert 257 <= len(ll_lens) <= 286 and 1 <= len(d_lens) <= 30
            assert expand_cl_seq(cl_seq) == list(ll_lens) + list(d_lens)
        if cl_lens is None:
            used = sorted(set(e[0] for e in cl_seq if e[0] != "bits"))
            if len(used) == 1:
                used.append(0 if used[0] != 0 else 1)
            cl_lens = assign(19, zip(used, complete_lengths(len(used))))
        need = max(i for i in range(19) if cl_lens[CL_ORDER[i]]) + 1
        hclen = max(need, 4) if hclen is None else hclen
        assert need <= hclen <= 19
        self.header(final, 2)
        w = self.w
        w.put((len(ll_lens) - 257) | ((len(d_lens) - 1) << 5) | ((hclen - 4) << 10), 14, COUNTS)
        for i in range(hclen):
            w.put(cl_lens[CL_ORDER[i]], 3, CL_TRIPLE)
        cl_codes = _revcodes(cl_lens)
        for e in cl_seq:
            if e[0] == "bits":                       # ("bits", value, width): a code the code-length alphabet does not have
                w.put(e[1], e[2], CL_SYM)
                continue
            c, n = cl_codes[e[0]]
            assert n, "code-length symbol %d has no code" % e[0]
            w.put(c, n, CL_SYM)
            if e[0] == 16:
                assert 3 <= e[1] <= 6
                w.put(e[1] - 3, 2, CL_EXTRA)
            elif e[0] == 17:
                assert 3 <= e[1] <= 10
                w.put(e[1] - 3, 3, CL_EXTRA)
            elif e[0] == 18:
                assert 11 <= e[1] <= 138
                w.put(e[1] - 11, 7, CL_EXTRA)
        self._tokens(tokens, _revcodes(ll_lens), _revcodes(d_lens), eob)
        return self

    def _tokens(self, tokens, ll, dd, eob):
        tokens = list(tokens)
        if eob and not (tokens and tokens[-1][0] == "eob"):
            tokens.append(("eob",))
        w = self.w
        put = w.put
        for t in tokens:
            t = as_raw(t)
            if t[0] == "lit":
                c, n = ll[t[1]]
                assert n, "literal %d has no code" % t[1]
                put(c, n, LIT)
            elif t[0] == "eob":
                c, n = ll[256]
                assert n, "no end-of-block code"
                put(c, n, EOB)
            elif t[0] == "bits":                     # ("bits", value, width, kind): anything the alphabets cannot say
                put(t[1], t[2], t[3])
            else:
                _, ls, lx, ds, dx = t
                c, n = ll[ls]
                assert n, "length symbol %d has no code" % ls
                put(c, n, LEN)
                put(lx, LEXTRA[ls - 257] if ls <= 285 else 0, LEN_EXTRA)
                if ds is not None:
                    c, n = dd[ds]
                    assert n, "distance symbol %d has no code" % ds
                    put(c, n, DIST)
                    put(dx, DEXTRA[ds] if ds <= 29 else 0, DIST_EXTRA)
        if self.out is not None:
            try:
                interpret(tokens, self.out)
            except ValueError:
                self.out = None

    # -- results --------------------------------------------------------------------------------------------------------------
    def payload(self):
        return self.w.getvalue()

    @property
    def nbits(self):
        return self.w.nbits


_FIXED_LL_CODES = _revcodes(FIXED_LL)
_FIXED_D_CODES = _revcodes(FIXED_D)


def fixed_filler_tokens(nbits):
    """literal tokens of a non-final fixed block that is exactly nbits long, header and end-of-block code included (nbits >= 82)"""
    body = nbits - 10
    nine = body % 8
    eight = (body - 9 * nine) // 8
    assert eight >= 0 and 8 * eight + 9 * nine == body
    return [("lit", 65 + i % 26) for i in range(eight)] + [("lit", 200 + i) for i in range(nine)]


def bgzf_wrap(payload, isize, crc):
    """a BGZF block around a raw DEFLATE payload with the trailer the caller claims (isize up to 65536, right or wrong)"""
    bsize = len(payload) + 26
    assert bsize <= 65536 and 0 <= isize <= 65536
    head = b"\x1f\x8b\x08\x04" + b"\0" * 4 + b"\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, bsize - 1)
    return head + payload + struct.pack("<II", crc & 0xffffffff, isize)


def bgzf_data(payload, data):
    return bgzf_wrap(payload, len(data), zlib.crc32(data))


def bgzf_filler(total_len, seed=0):
    """(block, data): a BGZF block of exactly total_len bytes holding one stored DEFLATE block - placed in front of a block it moves
    that block's payload to any address modulo 4"""
    n = total_len - 31
    assert n >= 1
    data = bytes((seed + 7 * i) & 0xff for i in range(n))
    s = Stream().stored(data, final=True)
    return bgzf_data(s.payload(), data), data


def place(blocks_with_residue, base_offset=0):
    """lay BGZF blocks out in one buffer so that each one's payload (18 bytes behind its start) lies at the requested address modulo 4
    (None: anywhere); fillers go in between.  -> (raw bytes, list of (kind, index, data) per block in file order), kind 'filler' or 'block'"""
    raw, order = bytearray(), []
    for i, (blk, res) in enumerate(blocks_with_residue):
        if res is not None:
            pad = (res - (base_offset + len(raw) + 18)) % 4
            if pad:
                f, data = bgzf_filler(32 + (pad - 32) % 4, seed=i)
                raw += f
                order.append(("filler", i, data))
            assert (base_offset + len(raw) + 18) % 4 == res
        raw += blk
        order.append(("block", i, None))
    return bytes(raw), order


def inflate_zlib(payload):
    """(bytes, eof, unused) of zlib's raw inflate; raises zlib.error"""
    d = zlib.decompressobj(-15)
    out = d.decompress(payload)
    return out, d.eof, d.unused_data


def straddles(log, boundaries):
    """per item: does one of the bit positions in `boundaries` lie strictly inside it"""
    kinds, off, w = log
    b = np.asarray(sorted(boundaries), dtype=np.int64)
    nxt = np.searchsorted(b, off, side="right")          # first boundary > off
    ok = nxt < len(b)
    hit = np.zeros(len(off), dtype=bool)
    hit[ok] = b[nxt[ok]] < (off + w)[ok]
    return hit
