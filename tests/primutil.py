"""What the tests of the shared primitives (csrc/scan.h, csrc/lines.h) share: the seams, taken from the library's own constants, seeded
case generators, so that the CPU and the GPU file see the same data, and the numpy statements of the operations they are held to."""
import itertools

import numpy as np

_cache = {}
GROUP, WAVE_BYTES = 16, 1024        # lines.h: bytes of text a thread takes, and a wave's 64 threads
WAVE_ELEMS, TRIP = 256, 4096        # scan.h: elements a wave takes at four a lane; elements k_scan_small takes a trip


def consts():
    if "c" not in _cache:
        from clairs_to_amd.primitives import constants
        _cache["c"] = constants()
    return _cache["c"]


def first_diff(got, want):
    """None when the arrays agree, else words for the assertion message"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return "shape / dtype %s %s, want %s %s" % (got.shape, got.dtype, want.shape, want.dtype)
    d = np.flatnonzero(got != want)
    if len(d) == 0:
        return None
    return "first difference at index %d: got %d, want %d (%d of %d differ)" % (d[0], got[d[0]], want[d[0]], len(d), len(want))


# ------------------------------------------------------------------------------------------------ scans
def scan_sizes():
    S = consts()["SCAN_TILE"]
    return sorted({0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, 4 * S - 1, 4 * S, 4 * S + 1,
                   5 * S - 1, 5 * S, 5 * S + 1, 1024 * S - 1, 1024 * S, 1024 * S + 1, 1025 * S + 5})


def group_sums(a, g):
    return np.add.reduceat(a.astype(np.int64), np.arange(0, len(a), g))


def assert_carries(name, a):
    """every wave, every trip of the one-workgroup loop and every tile adds something: a carry that is lost changes the output"""
    for g in sorted({WAVE_ELEMS, TRIP, consts()["SCAN_TILE"]}):
        assert np.all(group_sums(a, g) != 0), (name, len(a), g)


def _down_steps(n, rng):
    """+1 / -1 steps, -1 first and more often, with no wave, trip or tile that sums to nothing"""
    a = np.where(rng.random(n) < 0.3, 1, -1).astype(np.int32)
    a[0] = -1
    for _ in range(64):
        flipped = False
        for g in sorted({WAVE_ELEMS, TRIP, consts()["SCAN_TILE"]}):
            at = np.arange(0, n, g)
            for s in at[group_sums(a, g) == 0]:
                a[s + int(np.argmax(a[s:s + g] == 1))] = -1
                flipped = True
        if not flipped:
            break
    return a


def scan_families(n):
    """[(name, int32 vector, result types it is exact in)] for one length; read-only, and the last length asked for is kept"""
    if _cache.get("scan_n") != n:
        _cache["scan"] = None           # the old vectors go before the new ones are made
        _cache["scan"], _cache["scan_n"] = _scan_families(n), n
    return _cache["scan"]


def _scan_families(n):
    i32, i64 = np.int32, np.int64
    if n == 0:
        return [("empty", np.zeros(0, dtype=i32), (i32, i64))]
    rng = np.random.default_rng([20261021, n])
    out = [("ones", np.ones(n, dtype=i32), (i32, i64))]
    flags = rng.integers(0, 2, n, dtype=i32)
    flags[-1] = 1                       # the last wave's share may be one element
    if n < 2 * WAVE_ELEMS:
        flags[::64] = 1                 # short vectors: no wave's share without a flag
    out.append(("flags", flags, (i32, i64)))
    for name, at in (("first1", 0), ("last1", n - 1)):
        a = np.zeros(n, dtype=i32)
        a[at] = 1
        out.append((name, a, (i32, i64)))
    down = _down_steps(n, rng)
    assert np.cumsum(down, dtype=i64).min() < 0
    out.append(("down_steps", down, (i32, i64)))
    bound = max(2, (1 << 31) // n)
    small = rng.integers(1 if n < 1024 else 0, bound, n, dtype=i64).astype(i32)
    out.append(("below_2^31/n", small, (i32, i64)))
    exact = small.copy()
    exact[-1] += (1 << 31) - 1 - int(small.sum(dtype=i64))
    assert int(exact.sum(dtype=i64)) == (1 << 31) - 1 and exact[-1] >= small[-1]
    out.append(("total_2^31-1", exact, (i32, i64)))
    out.append(("up_to_2^31-1", rng.integers(0, 1 << 31, n, dtype=i64).astype(i32), (i64,)))
    for name, a, types in out:
        if name not in ("first1", "last1"):
            assert_carries(name, a)
        if i32 in types:
            assert np.abs(np.cumsum(a, dtype=i64)).max() < (1 << 31), name
        a.flags.writeable = False
    return out


def scan_reference(a, dtype):
    """numpy's running sum in int64, a zero in front; exact in `dtype` for the families that name it"""
    return np.concatenate((np.zeros(1, dtype=np.int64), np.cumsum(a, dtype=np.int64))).astype(dtype)


def pair_sizes():
    S = consts()["SCAN_TILE"]
    return [4 * S + 1, 1024 * S + 1]


# ------------------------------------------------------------------------------------------------ the tile scan
TILE_SCAN_SIZES = (1, 1023, 1024, 1025, 2048, 2049)


def tile_scan_case(n, stride):
    """int64 [n, stride]: values up to 2^40, every column drawn on its own and from its own range, so that a mixed-up stride shows"""
    rng = np.random.default_rng([20261022, n, stride])
    return np.stack([rng.integers(0, (1 << (40 - 2 * j)) + 1, n, dtype=np.int64) for j in range(stride)], axis=1)


def tile_scan_reference(a):
    c = np.cumsum(a, axis=0, dtype=np.int64)
    return np.concatenate((np.zeros((1, a.shape[1]), dtype=np.int64), c[:-1]), axis=0), c[-1].copy()


# ------------------------------------------------------------------------------------------------ line starts
def line_reference(text, cr):
    """byte 0, and every byte behind a '\\n' or, with cr, behind a '\\r' that is not itself followed by '\\n'"""
    t = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else np.asarray(text, dtype=np.uint8)
    if len(t) == 0:
        return np.zeros(0, dtype=np.uint32)
    ends = t[:-1] == 10
    if cr:
        ends |= (t[:-1] == 13) & (t[1:] != 10)
    return np.concatenate((np.zeros(1, dtype=np.int64), np.flatnonzero(ends) + 1)).astype(np.uint32)


ALPHABET = b"a\n\r"
PAIRS = b"aa\na\r\n\n\r\r"          # read round, every ordered pair of the alphabet once
assert {PAIRS[k:k + 1] + PAIRS[(k + 1) % 9:(k + 1) % 9 + 1] for k in range(9)} == {bytes(p) for p in itertools.product(ALPHABET, repeat=2)}
SHORT_EXHAUSTIVE, SHORT_MAX = 6, 33


def short_texts():
    """Texts of 1 .. 33 bytes over a, \\n and \\r.  Up to 6 bytes every string there is (1092 of them).  All 3^33 strings cannot be run,
    and need not be: whether byte i starts a line is a function of i, the length, and the bytes i - 1 and i alone (which of the sixteen
    bytes of a thread, which load path and which end of the text are i and the length; the text enters through that pair).  So from 7
    bytes on every length comes with nine texts, PAIRS read round from each of its nine places, which put every ordered pair of the
    alphabet on every byte i of every length: every value of (i, length, byte i - 1, byte i) is run."""
    for n in range(1, SHORT_EXHAUSTIVE + 1):
        for s in itertools.product(ALPHABET, repeat=n):
            yield bytes(s)
    for n in range(SHORT_EXHAUSTIVE + 1, SHORT_MAX + 1):
        for phase in range(9):
            yield bytes(PAIRS[(phase + k) % 9] for k in range(n))


def _base_text(n, rng):
    """lines of 'a' of 0 .. 78 bytes, three in ten ending in \\r\\n"""
    t = np.full(n, ord("a"), dtype=np.uint8)
    ends = np.cumsum(rng.integers(1, 80, n // 40 + 2))
    ends = ends[ends < n]
    t[ends] = 10
    crlf = ends[(rng.random(len(ends)) < 0.3) & (ends > 0)]
    t[crlf - 1] = 13
    return t


def _put(t, at, s):
    if at < 0 or at + len(s) > len(t):
        return False
    t[at:at + len(s)] = np.frombuffer(s, dtype=np.uint8)
    return True


def _seams(n, L):
    """offsets at which a 16-byte group, a wave's first thread and a tile begin, inside a text of n bytes"""
    return [b for b in (GROUP, 7 * GROUP, WAVE_BYTES, 5 * WAVE_BYTES + 0, L, 2 * L, 3000 * L, 4096 * L) if b < n]


def line_sizes():
    L = consts()["LINE_TILE"]
    return [L - 1, L, L + 1, 2 * L, 2 * L + 1]


def line_texts(n):
    """[(name, uint8 text)] of n bytes with what the line-start kernels can trip over planted at their seams"""
    L = consts()["LINE_TILE"]
    rng = np.random.default_rng([20261023, n])
    out = []
    # a line starting on the first byte of a group, of a wave and of a tile; a lone \r in the middle; a final \n
    t = _base_text(n, rng)
    seams = _seams(n, L)
    for b in seams:
        _put(t, b - 1, b"\na")
    _put(t, n // 2 - 1 + 3, b"a\ra")
    t[-1] = 10
    for cr in (0, 1):
        got = set(line_reference(t, cr).tolist())
        assert all(b in got for b in seams) and ((n // 2 + 4) in got) == bool(cr)
    out.append(("starts_on_seams", t))
    # \r\n cut by each of those seams; a lone \r as the last byte, unless a cut \r\n ends the text
    t = _base_text(n, rng)
    for b in seams:
        _put(t, b - 1, b"\r\n")
    if n - 1 not in seams:
        t[-2:] = (ord("a"), 13)
    got = set(line_reference(t, 1).tolist())
    assert all(b not in got and (b + 1 in got or b + 1 == n) for b in seams)
    out.append(("crlf_across_seams", t))
    # empty lines filling a whole tile (the second where there is one); no final \n
    t = _base_text(n, rng)
    tile = 1 if n >= 2 * L else 0
    t[max(0, tile * L - 1):min(n, (tile + 1) * L - 1)] = 10
    t[-1] = ord("a")
    assert np.count_nonzero(line_reference(t, 0) // L == tile) == min(L, n - tile * L)
    out.append(("tile_of_empty_lines", t))
    if n >= 2 * L:                      # one line over everything behind the first few bytes: tiles without a start
        t = np.full(n, ord("a"), dtype=np.uint8)
        _put(t, 3, b"\r\n")
        t[-1] = 10
        assert len(line_reference(t, 1)) == 2
        out.append(("tiles_without_a_start", t))
    return out


def big_line_text():
    """4096 tiles and a byte: sparse but for three tiles of empty lines, a line longer than two tiles, \\r\\n across a group, a wave and a
    tile seam, a start on the last tile's only byte, which is a lone \\r; about a million starts.  (text, {cr: its starts}), made once."""
    if "big" not in _cache:
        _cache["big"] = _big_line_text()
    return _cache["big"]


def _big_line_text():
    L = consts()["LINE_TILE"]
    n = 4096 * L + 1
    rng = np.random.default_rng([20261024, n])
    t = np.full(n, ord("a"), dtype=np.uint8)
    t[rng.integers(0, n, 800000)] = 10
    t[rng.integers(0, n, 60000)] = 13
    p = rng.integers(0, n - 1, 60000)
    t[p] = 13
    t[p + 1] = 10
    dense = (7, 2048, 4095)
    for tile in dense:
        t[tile * L - 1:(tile + 1) * L - 1] = 10
    t[100 * L + 50:102 * L + 150] = ord("a")
    _put(t, 3000 * L - 2, b"a\r\na")
    _put(t, 3000 * L + WAVE_BYTES - 2, b"a\r\na")
    _put(t, 3000 * L + 5 * GROUP - 2, b"a\r\na")
    _put(t, 3001 * L - 1, b"\na")
    t[-2:] = (10, 13)
    want = {}
    for cr in (0, 1):
        s = want[cr] = line_reference(t, cr)
        per_tile = np.bincount(s // L, minlength=4097)
        assert all(per_tile[k] == L for k in dense) and per_tile[101] == 0 and per_tile[4096] == 1 and 800000 < len(s) < 1300000
        got = set(s[(s >= 3000 * L - 2) & (s <= 3001 * L)].tolist())
        assert 3000 * L not in got and 3000 * L + 1 in got and 3001 * L in got
    t.flags.writeable = False
    return t, want
