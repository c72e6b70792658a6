"""The catalogue of hand-assembled DEFLATE streams for csrc/inflate.hip: named vectors, each with the branch of the kernel it is for.
Valid vectors carry the bytes the token interpreter gives (zlib has to agree: test_deflate_vectors.py); malformed ones the trailer they
claim and the status the kernel must end with.  The builders assert from the writer's event log that a vector contains what its name
says - a code of a given width, a window boundary inside an item - so nothing is left to the statistics of a text."""
import os
import re
import zlib
from collections import namedtuple

import numpy as np

from deflateutil import (CL_EXTRA, CL_SYM, CL_TRIPLE, DEXTRA, DIST, DIST_EXTRA, EOB, HDR, LEN, LEN_EXTRA, LEN_NLEN, LEXTRA, LIT, STORED,
                         Stream, assign, complete_lengths, fixed_filler_tokens, kraft, plain_cl_seq, stair_plus, staircase, straddles)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "clairs_to_amd", "csrc", "inflate.hip")) as _f:
    _src = _f.read()
TOK = int(re.search(r"#define\s+CTO_INF_TOK\s+(\d+)", _src).group(1))       # entries of the kernel's match queue
TBL = int(re.search(r"#define\s+CTO_INF_TBL\s+(\d+)", _src).group(1))       # index bits of its literal / length table
TBD = int(re.search(r"#define\s+CTO_INF_TBD\s+(\d+)", _src).group(1))       # ... and of its distance table
WINDOW_BITS = 2048        # the bit reader reloads its 64-dword input window at every 2048th bit, counted from the 4-byte-aligned base

# name, the branch it is for, payload, expected bytes (None: malformed), what zlib says ("ok" or why not), event log,
# claimed ISIZE and CRC-32, expected status (0, a code of bgzf.STATUS, None: any non-zero), weak: status != 0 OR CRC differs
Vector = namedtuple("Vector", "name note payload expected zlib_says log isize crc status weak")


def valid(name, note, s):
    assert s.out is not None, name
    out = bytes(s.out)
    assert 1 <= len(out) <= 65536, (name, len(out))
    return Vector(name, note, s.payload(), out, "ok", s.w.log(), len(out), zlib.crc32(out), 0, False)


def malformed(name, note, s, zlib_says, claimed, status, weak=False, cut=0):
    p = s.payload()
    return Vector(name, note, p[:len(p) - cut] if cut else p, None, zlib_says, s.w.log(), len(claimed), zlib.crc32(claimed), status, weak)


def widths(log, kind):
    k, _, w = log
    return set(int(x) for x in w[k == kind])


def lits(b):
    return [("lit", x) for x in bytes(b)]


SHORT_D = [1, 1]                                             # distances 1 and 2 on one bit each


def stair_ll(special, n=16, n_syms=286):
    """literal / length lengths 1, 2, ..., n-1, n-1: `special` {symbol: length} placed as asked, letters from 'a' on the other codes"""
    slots = staircase(n)
    pairs = []
    for sym, l in special.items():
        slots.remove(l)
        pairs.append((sym, l))
    filler = [c for c in range(97, 97 + n) if c not in special][:len(slots)]
    pairs += list(zip(filler, slots))
    return assign(n_syms, pairs), filler


# ---- A: code lengths across the table boundary ----------------------------------------------------------------------------------
def group_a():
    out = []
    for lit_len, len_len, eob_len in ((9, 10, 15), (10, 15, 9), (15, 9, 10)):
        ll, filler = stair_ll({90: lit_len, 258: len_len, 256: eob_len})
        toks = lits(filler) + [("lit", 90), ("match", 4, 1), ("lit", 90), ("match", 4, 2)] + lits(filler[::-1]) + [("match", 4, 1)]
        s = Stream().dynamic(toks, ll, SHORT_D, final=True)
        v = valid("A/ll-stair lit%d len%d eob%d" % (lit_len, len_len, eob_len),
                  "R_RARE: literal, length and end-of-block on codes of 9 / 10 / 15 bits; every code length 1..15 in use", s)
        assert lit_len in widths(v.log, LIT) and len_len in widths(v.log, LEN) and eob_len in widths(v.log, EOB), v.name
        assert widths(v.log, LIT) | widths(v.log, LEN) | widths(v.log, EOB) == set(range(1, 16)), v.name
        out.append(v)
    # distances on 1..15 bits behind lengths that hit the table
    d_stair = staircase(16)
    ll = assign(286, zip([97, 98, 99, 100, 101, 102, 256, 257, 264, 285], complete_lengths(10)))
    body = lits(b"abcdef" * 50)
    toks = body + [("raw", (257, 264, 285)[ds % 3], 0, ds, (1 << DEXTRA[ds]) - 1) for ds in range(16)]
    s = Stream().dynamic(toks, ll, d_stair, final=True)
    v = valid("A/dist-stair", "R_RARE_DIST: table-hit lengths, distances on codes of 1..15 bits (8, 9 and 15 among them)", s)
    assert widths(v.log, DIST) == set(range(1, 16)) and max(widths(v.log, LEN)) <= TBL, v.name
    out.append(v)
    # long length, then long distance
    ll, filler = stair_ll({90: 9, 258: 15, 265: 14, 256: 10})
    toks = lits(bytes(filler) * 20) + [("raw", (258, 265)[ds & 1], ds & 1, ds, 0) for ds in range(16)] + [("lit", 90)]
    s = Stream().dynamic(toks, ll, d_stair, final=True)
    v = valid("A/long-length-long-distance", "R_RARE -> slow_dist -> canonical search for both codes of a match", s)
    k, _, w = v.log
    idx = np.nonzero(k == LEN)[0]
    nxt = [int(w[np.nonzero(k[i:] == DIST)[0][0] + i]) for i in idx]
    assert any(int(w[i]) > TBL and d > TBD for i, d in zip(idx, nxt)) and any(int(w[i]) > TBL and d == 15 for i, d in zip(idx, nxt)), v.name
    out.append(v)
    return out


# ---- B: every symbol's arithmetic -----------------------------------------------------------------------------------------------
def b_tokens():
    L = [(257 + i, x) for i in range(29) for x in sorted({0, (1 << LEXTRA[i]) - 1})]
    D = [(i, x) for i in range(30) for x in sorted({0, (1 << DEXTRA[i]) - 1})]
    assert (284, 31) in L and (285, 0) in L            # length 258 the long way and the short way
    n = max(len(L), len(D))
    toks = [("raw",) + L[i % len(L)] + D[i % len(D)] for i in range(n)]
    assert set(t[1:3] for t in toks) == set(L) and set(t[3:5] for t in toks) == set(D)
    return toks


def group_b():
    out = []
    rng = np.random.default_rng(1951)
    window = bytes(rng.integers(0, 256, 32768, dtype=np.uint8))
    first = [("match", 258, 32768)]                    # source offset 0: the stored block's first byte
    s = Stream().stored(window).fixed(first + b_tokens(), final=True)
    out.append(valid("B/all-symbols fixed", "len_code / dist_code: every length and distance symbol at its smallest and largest "
                     "extra bits through the tables; matches read a stored block's output", s))
    # the same tokens with every length symbol, and 23 of the 30 distance symbols at a time, on codes longer than the tables' index
    ll = assign(286, [(0, 1), (256, 2)] + [(i, 10) for i in range(1, 228)] + [(i, 10) for i in range(257, 286)])
    short, longs = stair_plus(7, 23)
    for name, d_lens in (("low distances short", short + longs), ("high distances short", longs + short[::-1])):
        assert kraft(ll) == 1 and kraft(d_lens) == 1 and len(d_lens) == 30
        s = Stream().stored(window).dynamic(first + [("lit", 0)] + b_tokens(), ll, d_lens, final=True)
        v = valid("B/all-symbols long codes, " + name, "litlen_entry / dist_entry behind huff_decode: HLIT = 286, all 30 distance codes, "
                  "length codes of 10 bits, distance codes of 11 and 12 bits", s)
        assert widths(v.log, LEN) == {10} and max(widths(v.log, DIST)) > TBD, v.name
        out.append(v)
    s = Stream().fixed(lits(b"abcdefgh") + [("match", 5, 8), ("match", 20, 13), ("match", 258, 33)], final=True)
    out.append(valid("B/distance equals output so far", "queue_match's d > vop bound: source offset 0 with a length below and above the distance", s))
    return out


# ---- C: degenerate alphabets ----------------------------------------------------------------------------------------------------
def group_c():
    out = []
    ll8 = assign(257, zip([97, 98, 99, 100, 101, 102, 103, 256], complete_lengths(8)))
    s = Stream().dynamic(lits(b"abcdefgfedcba" * 9), ll8, [0], final=True)
    out.append(valid("C/no distance code", "huff_build<1>(hd) over all-zero lengths (HDIST = 1, HLIT = 257): literals only", s))
    llm = assign(260, zip([97, 98, 99, 100, 256, 257, 258, 259], complete_lengths(8)))
    toks = lits(b"a") + [("match", 3 + i % 3, 1) for i in range(150)]
    s = Stream().dynamic(toks, llm, [1], final=True)
    out.append(valid("C/one distance code of one bit", "an incomplete distance code is legal: one code, used by 150 matches", s))
    toks = lits(b"abcdabcd") + [("match", 3 + i % 3, 5 + i % 2) for i in range(60)]
    s = Stream().dynamic(toks, llm, [0, 0, 0, 0, 1], final=True)
    out.append(valid("C/one distance code, symbol 4", "one code whose symbol has an extra bit (distances 5 and 6)", s))
    toks = lits(b"abcd") + [("match", 3 + i % 3, 1 + i % 2) for i in range(60)]
    s = Stream().dynamic(toks, llm, [1, 1], final=True)
    out.append(valid("C/two distance codes", "the smallest distance alphabet zlib writes", s))
    ll, filler = stair_ll({256: 10, 255: 10}, n=11, n_syms=257)
    s = Stream().dynamic(lits(bytes(filler) * 7), ll, [0], final=True)
    v = valid("C/only long code is end-of-block", "R_RARE reached by the end-of-block code alone; every literal hits the table", s)
    assert max(widths(v.log, LIT)) <= TBL and widths(v.log, EOB) == {10}, v.name
    out.append(v)
    return out


# ---- D: code-length header ------------------------------------------------------------------------------------------------------
def d1_block(s, final):
    """HCLEN = 19; 18 with 138 and 11 repeats, 17 with 10 and 3, 16 with 6 and 3 repeating a 15, an 18-run that crosses from the
    literal / length lengths into the distance lengths"""
    ll = [0] * 162 + [15] * 10 + list(range(1, 12)) + [0] * 73 + [13, 14] + [0] * 28
    d = [0, 0, 0, 1, 1]
    seq = [(18, 138), (18, 11), (17, 10), (17, 3), (15,), (16, 6), (16, 3)] + plain_cl_seq(range(1, 12)) + [(18, 73), (13,), (14,), (18, 31), (1,), (1,)]
    assert kraft(ll) == 1 and len(ll) == 286
    toks = lits(range(162, 183)) + [("raw", 257, 0, 3, 0), ("raw", 257, 0, 4, 1)]
    return s.dynamic(toks, ll, d, final=final, cl_seq=seq, hclen=19)


def group_d():
    out = []
    out.append(valid("D/runs 18x138 18x11 17x10 17x3 16x6 16x3, 18-run across HLIT", "the code-length loop: all three lane / lane + 64 / "
                     "lane + 128 writes, a repeated 15, a zero run from the literal / length into the distance lengths, HCLEN = 19",
                     d1_block(Stream(), True)))
    ll = assign(286, [(97 + i, 1 + i) for i in range(12)] + [(109, 14), (256, 13), (285, 14)])
    d = [14] * 4 + list(range(1, 13))
    seq = ([(18, 97)] + plain_cl_seq(range(1, 13)) + [(14,), (18, 138), (17, 8), (13,), (18, 28), (14,), (16, 4)] + plain_cl_seq(range(1, 13)))
    assert kraft(ll) == 1 and kraft(d) == 1
    toks = lits(b"abcdefghijklmabcdefg") + [("raw", 285, 0, ds, 0) for ds in (0, 1, 2, 3, 4, 5, 8)]
    s = Stream().dynamic(toks, ll, d, final=True, cl_seq=seq)
    out.append(valid("D/16-run across HLIT", "a 16-run that repeats the last literal / length length into the first four distance lengths", s))
    ll = [6] * 32 + [7] * 32 + [8] * 32 + [9] * 63 + [0] * 97 + [9]
    assert kraft(ll) == 1
    cl = assign(19, zip([0, 6, 7, 8, 9, 16, 17, 18], staircase(8)))
    s = Stream().dynamic(lits(range(0, 159, 3)), ll, [0], final=True, cl_lens=cl)
    v = valid("D/7-bit code-length codes, 8 triples", "huff_decode<1>(hc) on codes of 1..7 bits; HCLEN field 4", s)
    assert 7 in widths(v.log, CL_SYM) and int((v.log[0] == CL_TRIPLE).sum()) == 8, v.name
    out.append(v)
    # four triples can only name the symbols 16, 17, 18 and 0 - no code at all; five is the least a valid header can have
    ll = [8] * 255 + [0, 8]
    s = Stream().dynamic(lits(range(255)), ll, [0], final=True, cl_seq=plain_cl_seq(ll + [0]), cl_lens=assign(19, [(0, 1), (8, 1)]), hclen=5)
    v = valid("D/5 triples", "the shortest HCLEN a valid block can have (4 triples cannot give any symbol a code); no repeat symbol at all", s)
    assert int((v.log[0] == CL_TRIPLE).sum()) == 5, v.name
    out.append(v)
    ll8 = assign(257, zip([97, 98, 99, 100, 101, 102, 103, 256], complete_lengths(8)))
    s = Stream().dynamic(lits(b"gfedcba"), ll8, [0], final=True, hclen=19)
    out.append(valid("D/19 triples, trailing zeros", "HCLEN = 19 where the last triples are zero", s))
    return out


# ---- E: block sequences inside one BGZF block -----------------------------------------------------------------------------------
def group_e():
    out = []
    rng = np.random.default_rng(5)
    ll_long, filler = stair_ll({256: 15, 258: 14})
    ll_short = assign(286, zip([97, 98, 99, 100, 256, 257, 258, 259], complete_lengths(8)))
    s = Stream()
    for i in range(200):
        final = i == 199
        if i % 3 == 0:
            s.stored(bytes(rng.integers(0, 256, int(rng.integers(0, 20)), dtype=np.uint8)), final=final)
        elif i % 3 == 1:
            s.fixed(lits(b"xy") + ([("match", 3 + i % 7, 1 + i % 2)] if i > 3 else []), final=final)
        elif i % 2:
            s.dynamic(lits(bytes(filler[:5 + i % 9])) + [("match", 4, 2)], ll_long, SHORT_D, final=final)
        else:
            s.dynamic(lits(b"abcd") + [("match", 3, 4), ("match", 5, 2 + i % 5)], ll_short, [3, 3, 3, 3, 3, 3, 3, 3], final=final)
    out.append(valid("E/200 blocks stored fixed dynamic", "the block loop: tables, sorted[] and the bit reader carried over 200 block headers", s))
    s = Stream()
    for i in range(6):
        if i % 2 == 0:
            s.dynamic(lits(bytes(filler)) + [("match", 4, 3 + i)], ll_long, staircase(16), final=i == 5)
        else:
            s.dynamic(lits(b"abcdabcd") + [("match", 5, 2)], ll_short, SHORT_D, final=i == 5)
    s2 = Stream()
    for i in range(6):
        if i % 2 == 1:
            s2.dynamic(lits(bytes(filler)) + [("match", 4, 3 + i)], ll_long, staircase(16), final=i == 5)
        else:
            s2.dynamic(lits(b"abcdabcd") + [("match", 5, 2)], ll_short, SHORT_D, final=i == 5)
    out.append(valid("E/dynamic long then short alphabets", "huff_build / huff_table32 over the previous block's LDS tables and sorted[]", s))
    out.append(valid("E/dynamic short then long alphabets", "the reverse order", s2))
    seen = set()
    for p in range(8):
        s = Stream().fixed(fixed_filler_tokens(88 + p))                       # the next header starts at bit phase p
        s.stored(b"")
        s.fixed(fixed_filler_tokens(88 + (p - s.nbits) % 8 + 3))              # ... and the final empty block at phase (p + 3) % 8
        s.stored(b"", final=True)
        v = valid("E/empty stored blocks at bit phase %d" % p, "the stored path's alignment drop with LEN = 0, non-final and final", s)
        k, off, _ = v.log
        hdrs = np.nonzero(k == HDR)[0]
        seen.add(("nonfinal", int(off[hdrs[1]]) % 8))
        seen.add(("final", int(off[hdrs[3]]) % 8))
        out.append(v)
    assert seen == set((f, p) for f in ("nonfinal", "final") for p in range(8)), sorted(seen)
    s = Stream().fixed([]).dynamic([], ll_short, SHORT_D).fixed(lits(b"after"), final=True)
    out.append(valid("E/blocks of an end-of-block code only", "R_EOB as the first symbol of a non-final fixed and dynamic block", s))
    toks = lits(b"0123456789") + [("match", 3 + i, 2 + i) for i in range(8)]
    s = Stream().fixed(toks).stored(b"STOREDBYTES").fixed([("match", 11, 11), ("match", 6, 30)], final=True)
    out.append(valid("E/stored block behind queued matches", "resolve_matches at block end; a later match copies the stored bytes", s))
    return out


# ---- F: input-window boundaries -------------------------------------------------------------------------------------------------
F_KINDS = [LIT, LEN, LEN_EXTRA, "gap", DIST, DIST_EXTRA, CL_TRIPLE, CL_SYM, CL_EXTRA, LEN_NLEN, STORED]


def window_hits(log, residue):
    """the F_KINDS an input-window boundary falls into when the payload lies at address `residue` modulo 4: strictly inside an item's
    bits; "gap": between a length and its distance (the boundary is the distance code's first bit); stored data: between two bytes"""
    k, off, w = log
    total = int(off[-1] + w[-1])
    bounds = [b for b in range(WINDOW_BITS - 8 * residue, total, WINDOW_BITS)]
    if not bounds:
        return set()
    inside = straddles(log, bounds)
    hits = set(int(x) for x in k[inside]) & set(x for x in F_KINDS if not isinstance(x, str))
    at = np.isin(off, bounds)
    if (at & (k == DIST)).any():
        hits.add("gap")
    prev_stored = np.concatenate([[False], k[:-1] == STORED])
    if (at & (k == STORED) & prev_stored).any():
        hits.add(STORED)
    return hits


def group_f():
    out = []
    # symbols: wide literal, length and distance codes with extra bits, shifted through 64 bit phases
    ll, filler = stair_ll({90: 15, 281: 13, 265: 14, 256: 12})
    d = assign(12, [(0, 1), (1, 2), (9, 3), (10, 4), (11, 4)])
    assert kraft(d) == 1
    cycle = [("lit", 90), ("raw", 281, 21, 10, 9), ("lit", filler[0]), ("raw", 265, 1, 11, 14), ("lit", 90), ("raw", 281, 30, 9, 5)]
    toks = lits(bytes(filler) * 5) + cycle * 120
    for shift in range(64):
        s = Stream().fixed(fixed_filler_tokens(82 + shift)).dynamic(toks, ll, d, final=True)
        out.append(valid("F/symbols behind %d bits" % (82 + shift), "the assembly's two refills and R_REFILL / R_RARE_DIST at a window reload", s))
    # headers: HCLEN triples, code-length symbols and their repeat bits around bit 2048
    for p in range(1700, 2040, 7):
        s = d1_block(Stream().fixed(fixed_filler_tokens(p)), True)
        out.append(valid("F/dynamic header behind %d bits" % p, "bits_refill's reload inside the HCLEN triples / the code-length loop", s))
    # stored: LEN / NLEN and data
    for j in range(64):
        s = Stream().fixed(fixed_filler_tokens(1602 + 8 * j)).stored(bytes(range(65, 125))).fixed([("match", 60, 60)], final=True)
        out.append(valid("F/stored block behind %d bits" % (1602 + 8 * j), "bits_refill's reload inside LEN / NLEN and the stored copy loop", s))
    missing = [(k, r) for r in range(4) for k in F_KINDS if not any(k in window_hits(v.log, r) for v in out)]
    assert not missing, "no vector has a window boundary in: %r" % (missing,)
    return out


# ---- G: the match queue ---------------------------------------------------------------------------------------------------------
def n_matches(log):
    return int((log[0] == DIST).sum())


def group_g():
    out = []
    head = lits(b"0123456789")
    for n in (TOK - 1, TOK, TOK + 1):
        s = Stream().fixed(head + [("match", 3 + i % 6, 1 + i % 9) for i in range(n)], final=True)
        v = valid("G/%d matches then end of block" % n, "R_QUEUE / resolve_matches at block end with the queue one short of full, full, one over", s)
        assert n_matches(v.log) == n
        out.append(v)
    s = Stream().fixed(head + [("match", 3 + i % 6, 1 + i % 9) for i in range(TOK)]).stored(b"stored").fixed([("match", 9, 8)], final=True)
    out.append(valid("G/%d matches then a stored block" % TOK, "an empty queue at the end-of-block code, then the stored path", s))
    toks = lits(bytes(i & 0xff for i in range(200))) + [("match", 3, 200 + 3 * i - 2 * i) for i in range(100)]
    s = Stream().fixed(toks, final=True)
    out.append(valid("G/100 independent matches", "resolve_matches: one round takes a whole 64-lane window", s))
    for d in (1, 2):
        s = Stream().fixed(lits(b"xy") + [("match", 3 + i % 4, d) for i in range(300)], final=True)
        out.append(valid("G/chain of 300 matches at distance %d" % d, "resolve_matches: every match waits for the one before it, one round each", s))
    toks = lits(b"abcdef") + [("match", 4, 3), ("lit", 81), ("match", 5, 1), ("lit", 82), ("match", 3, 8), ("match", 4, 2)]
    s = Stream().fixed(toks, final=True)
    out.append(valid("G/source is a literal behind a pending match", "the `ready` rule: a final byte above the oldest unresolved destination", s))
    toks = lits(bytes((i * 7 + 1) & 0xff for i in range(257))) + [("match", 258, 1), ("match", 258, 2), ("match", 258, 3), ("match", 258, 257)]
    s = Stream().fixed(toks, final=True)
    out.append(valid("G/overlapping copies of 258 bytes at distance 1, 2, 3, 257", "the (k mod d) copy; the last match ends exactly at ISIZE", s))
    ll, filler = stair_ll({90: 15, 258: 3, 256: 15})
    s = Stream().dynamic(lits(bytes(filler)) + [("match", 4, 2), ("lit", 90)], ll, SHORT_D, final=True)
    v = valid("G/last byte is a literal on a 15-bit code", "R_RARE's literal store at vop = isize - 1", s)
    assert v.log[0][-2] == LIT and v.log[2][-2] == 15
    out.append(v)
    return out


# ---- H: sizes -------------------------------------------------------------------------------------------------------------------
def group_h():
    out = []
    out.append(valid("H/ISIZE 1", "the smallest block that is not the end-of-file marker", Stream().fixed(lits(b"A"), final=True)))
    rng = np.random.default_rng(8)
    s = Stream().stored(bytes(rng.integers(0, 256, 32768, dtype=np.uint8)))
    s.fixed([("match", 258, 32768)] * 126 + [("match", 4, 32768)], final=True)
    v = valid("H/ISIZE 65280", "what BGZF writers put into one block", s)
    assert v.isize == 65280
    out.append(v)
    s = Stream().fixed([("lit", 0)] + [("match", 258, 1)] * 254 + [("match", 3, 1)], final=True)
    v = valid("H/ISIZE 65536", "the 16-bit destination and source fields of a queue entry at their limit", s)
    assert v.isize == 65536 and v.expected == b"\0" * 65536
    out.append(v)
    return out


def valid_vectors():
    out = group_a() + group_b() + group_c() + group_d() + group_e() + group_f() + group_g() + group_h()
    assert len(set(v.name for v in out)) == len(out)
    return out


# ---- malformed streams ----------------------------------------------------------------------------------------------------------
def malformed_vectors():
    out = []
    ll8 = assign(257, zip([97, 98, 99, 100, 101, 102, 103, 256], complete_lengths(8)))
    llm = assign(260, zip([97, 98, 99, 100, 256, 257, 258, 259], complete_lengths(8)))
    s = Stream()
    s.header(True, 3)
    s.w.put(0x155, 13, HDR)
    out.append(malformed("M/block type 3", "ST_BAD_BTYPE", s, "error", b"abc", 1))
    s = Stream().fixed(lits(b"ab")).stored(b"hello", final=True, nlen=0x1234)
    out.append(malformed("M/stored NLEN mismatch", "ST_BAD_STORED", s, "error", b"abhello", 2))
    s = Stream().dynamic(lits(b"ab"), assign(257, [(97, 1), (98, 1), (256, 1)]), [0], final=True)
    out.append(malformed("M/over-subscribed literal/length set", "ST_BAD_TABLE from huff_build<5>(hl)", s, "error", b"ab", 3))
    s = Stream().dynamic(lits(b"abc"), ll8, [0], final=True, cl_seq=[(16, 3)] + plain_cl_seq(ll8[3:] + [0]), check=False)
    out.append(malformed("M/symbol 16 first", "ST_BAD_TABLE: nothing to repeat", s, "error", b"abc", 3))
    s = Stream().dynamic(lits(b"abc"), ll8, [0], final=True, cl_seq=plain_cl_seq(ll8[:250]) + [(18, 138)], check=False)
    out.append(malformed("M/repeat past HLIT + HDIST", "ST_BAD_TABLE: i + rep > total", s, "error", b"abc", 3))
    s = Stream().fixed(lits(b"abc") + [("raw", 286, 0, None, 0)], final=True)
    out.append(malformed("M/length symbol 286 in a fixed block", "ST_BAD_CODE through E_BAD", s, "error", b"abcabc", 4))
    s = Stream().fixed(lits(b"abc") + [("raw", 257, 0, 30, 0)], final=True)
    out.append(malformed("M/distance symbol 30 in a fixed block", "ST_BAD_DIST: a 5-bit code behind the 30 symbols", s, "error", b"abcabc", 5))
    s = Stream().dynamic(lits(b"abc") + [("match", 3, 1), ("raw", 257, 0, None, 0), ("bits", 1, 1, DIST)], llm, [1], final=True)
    out.append(malformed("M/unused code of a one-code distance alphabet", "ST_BAD_DIST from slow_dist's canonical search", s, "error", b"abcccccc", 5))
    s = Stream().fixed(lits(b"abcde") + [("match", 3, 6)], final=True)
    out.append(malformed("M/distance one more than the output so far", "ST_BAD_DIST from the d > vop bound", s, "error", b"abcdeabc", 5))
    s = Stream().fixed(lits(b"abcdefghij"), final=True)
    out.append(malformed("M/one literal more than ISIZE", "ST_OVERRUN_OUT at the end of the block", s, "long", b"abcdefghi", 6))
    s = Stream().fixed(lits(b"abcdef") + [("match", 4, 3)], final=True)
    out.append(malformed("M/a match one byte past ISIZE", "ST_OVERRUN_OUT from the match's exact bound", s, "long", b"abcdefdef", 6))
    s = Stream().fixed(lits(b"abcdef") + [("match", 4, 3)], final=True)
    out.append(malformed("M/less output than ISIZE", "ST_SHORT", s, "short", b"abcdefdefdX", 8))
    text = bytes(33 + (i * 37) % 90 for i in range(400))
    s = Stream().fixed(lits(text), final=True)
    out.append(malformed("M/payload cut off before its end-of-block code", "the zeros behind `limit`: any status but 0", s, "truncated", text, None, cut=60))
    # where the kernel was or is more lenient than zlib
    s = Stream().dynamic(lits(b"abc") + [("match", 3, 1)], llm, [1, 1, 1], final=True)
    out.append(malformed("L/over-subscribed distance set", "ST_BAD_TABLE from huff_build<1>(hd)'s verdict", s, "error", b"abcccc", 3))
    s = Stream().dynamic(lits(b"abc"), ll8, [0], final=True, cl_seq=plain_cl_seq(ll8[:200]) + [("bits", 7, 3)] + plain_cl_seq(ll8[201:] + [0]),
                         cl_lens=assign(19, [(0, 1), (3, 2), (7, 3)]), check=False)
    out.append(malformed("L/incomplete code-length set, unused code in use", "stays lenient at the table; the code 111 names no symbol", s,
                         "error", b"abc", None, weak=True))
    s = Stream().dynamic(lits(b"ab") + [("bits", 7, 3, LIT)] + lits(b"ab"), assign(257, [(97, 1), (98, 2), (256, 3)]), [0], final=True)
    out.append(malformed("L/incomplete literal/length set, unused code in use", "stays lenient at the table; the code 111 names no symbol", s,
                         "error", b"abab", None, weak=True))
    assert len(set(v.name for v in out)) == len(out)
    return out
