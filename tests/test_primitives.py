"""The shared primitives without a GPU: the host loops of csrc/primitives.hip, which state what the prefix sums (csrc/scan.h), the tile scan
and the line starts (csrc/lines.h) are, against numpy at the seams of the kernels, and the library's constants against the headers' own
lines.  tests/test_gpu_primitives.py holds the kernels to numpy on the same data through the check_* functions below."""
import os
import re

import numpy as np
import pytest

import primutil as pu
from conftest import ROOT

C = pu.consts()
LARGE = 1024 * C["SCAN_TILE"] - 1
THINNED = ("flags", "down_steps", "total_2^31-1", "up_to_2^31-1")     # what the host loop runs at the four largest lengths


def test_constants_are_the_headers_own_lines():
    seen = {}
    for header in ("scan.h", "sort.h", "lines.h"):
        src = open(os.path.join(ROOT, "clairs_to_amd", "csrc", header)).read()
        for line in re.findall(r"^constexpr (?:int|int64_t) ([^;]+);", src, flags=re.M):
            for name, expr in re.findall(r"(\w+) = ([^,]+)", line):
                seen[name] = int(eval(expr.replace("int64_t(1)", "1"), {"__builtins__": {}}, dict(seen)))
    assert {k: seen[k] for k in C} == C
    assert C["SCAN_TILE"] == pu.TRIP and C["SORT_MAX_N"] == 1 << 30


def check_scan(n, where, only=None):
    from clairs_to_amd.primitives import scan
    for name, a, types in pu.scan_families(n):
        if only is not None and name not in only:
            continue
        for dt in types:
            want = pu.scan_reference(a, dt)
            for form in ((0, 1) if dt is np.int32 else (0,)):
                for with_total in (True, False):
                    out, total = scan(a, dt, form, where, with_total=with_total)
                    case = "scan of %s, n = %d, %s, form %d, %s total pointer" % (name, n, np.dtype(dt).name, form, "with a" if with_total else "no")
                    d = pu.first_diff(out, want)
                    assert d is None, "%s: %s" % (case, d)
                    assert total == (int(want[-1]) if with_total else None), case


def check_scan_pair(n, where):
    """two different vectors, one scan right behind the other on one stream and one scratch"""
    from clairs_to_amd.primitives import scan
    fam = {name: a for name, a, _ in pu.scan_families(n)}
    a, b = fam["flags"], fam["total_2^31-1"]
    for dt, form in ((np.int32, 0), (np.int64, 0), (np.int32, 1)):
        for x, y in ((a, b), (b, a)):
            got = scan(x, dt, form, where, second=y)
            for k, v in enumerate((x, y)):
                want = pu.scan_reference(v, dt)
                case = "scan pair, n = %d, %s, form %d, vector %d" % (n, np.dtype(dt).name, form, k)
                d = pu.first_diff(got[k][0], want)
                assert d is None, "%s: %s" % (case, d)
                assert got[k][1] == int(want[-1]), case


def check_tile_scan(where):
    from clairs_to_amd.primitives import scan_tiles
    for stride in (1, 2, 3):
        for n in pu.TILE_SCAN_SIZES:
            a = pu.tile_scan_case(n, stride)
            before = a.copy()
            want, want_totals = pu.tile_scan_reference(a)
            got, totals = scan_tiles(a, where)
            assert np.array_equal(a, before)
            for j in range(stride):
                case = "tile scan, n = %d, stride %d, column %d" % (n, stride, j)
                d = pu.first_diff(got[:, j], want[:, j])
                assert d is None, "%s: %s" % (case, d)
                assert totals[j] == want_totals[j], case


def check_lines(name, text, where, want=None):
    from clairs_to_amd.primitives import line_starts
    for cr in (0, 1):
        ref = want[cr] if want is not None else pu.line_reference(text, cr)
        d = pu.first_diff(line_starts(text, cr, where), ref)
        assert d is None, "line starts of %s, %d bytes, cr = %d: %s" % (name, len(text), cr, d)


def check_short_lines(where):
    n = 0
    for text in pu.short_texts():
        check_lines(repr(text), text, where)
        n += 1
    assert n == sum(3 ** k for k in range(1, pu.SHORT_EXHAUSTIVE + 1)) + 9 * (pu.SHORT_MAX - pu.SHORT_EXHAUSTIVE)


def check_sized_lines(n, where):
    texts = pu.line_texts(n)
    assert len(texts) == (4 if n >= 2 * C["LINE_TILE"] else 3)
    for name, text in texts:
        assert len(text) == n
        check_lines(name, text, where)


def check_big_lines(where):
    text, want = pu.big_line_text()
    check_lines("4096 tiles and a byte", text, where, want)


@pytest.mark.parametrize("n", pu.scan_sizes())
def test_host_scan_is_numpys_running_sum(n):
    check_scan(n, "host", THINNED if n >= LARGE else None)


def test_host_scans_back_to_back():
    for n in pu.pair_sizes():
        check_scan_pair(n, "host")


def test_host_tile_scan_is_numpys_running_sum():
    check_tile_scan("host")


def test_host_line_starts_of_every_short_text():
    check_short_lines("host")


@pytest.mark.parametrize("n", pu.line_sizes())
def test_host_line_starts_around_the_tile(n):
    check_sized_lines(n, "host")


def test_host_line_starts_of_64_mib():
    check_big_lines("host")


def test_what_the_entries_refuse():
    from clairs_to_amd._lib import CtoError
    from clairs_to_amd.primitives import scan, scan_tiles
    with pytest.raises(CtoError):
        scan(np.ones(4, dtype=np.int32), np.int64, 1, "host")          # in place is int32 only
    with pytest.raises(CtoError):
        scan_tiles(np.ones((4, 4), dtype=np.int64), "host")
    out, total = scan(np.zeros(0, dtype=np.int32), np.int64, 0, "host")
    assert out.tolist() == [0] and total == 0
