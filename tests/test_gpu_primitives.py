"""The kernels every device command rests on, at their own seams: scan_exclusive and k_scan_small in place (csrc/scan.h), k_scan_tiles, and the
line-start passes (csrc/lines.h), through the entries of csrc/primitives.hip and against numpy on the data of tests/primutil.py, which
tests/test_primitives.py runs through the host loops.  Those entries compile their own copy of the kernels, as every user does, so the
seams are crossed again where production crosses them: cto_candidate_positions' in-place scan here, add_back's sort and scans in
tests/test_gpu_add_back.py.  The sort's own cases are test_add_back.sort_cases."""
import types

import numpy as np
import pytest

import primutil as pu
from test_primitives import C, check_big_lines, check_lines, check_scan, check_scan_pair, check_short_lines, check_sized_lines, check_tile_scan

pytestmark = pytest.mark.gpu
S = C["SCAN_TILE"]


def test_buffers_that_regrow_between_calls():
    """small, the largest case, small again, in one process and from no buffers at all: the grow-only buffers are reallocated between
    the calls and an address kept from before would show.  (cto_sort_u64 keeps its buffers for the life of the process; sort_cases'
    lengths ascend, so they regrow from one length to the next there, under results that are all checked.)"""
    from clairs_to_amd.add_back_missing_variants_in_genotyping import sort_u64
    from clairs_to_amd.primitives import release
    release()
    rng = np.random.default_rng(20261025)
    big_text, big_want = pu.big_line_text()
    small_text = pu.line_texts(C["LINE_TILE"] + 1)[0]
    for n_scan, n_sort, (name, text), want in ((257, 65, small_text, None), (1025 * S + 5, 192 * C["SORT_TILE"] + 77, ("64 MiB", big_text), big_want),
                                               (257, 65, small_text, None), (5 * S + 1, 3 * C["SORT_TILE"] + 7, small_text, None)):
        check_scan(n_scan, "device", ("flags", "up_to_2^31-1"))
        check_scan_pair(n_scan, "device")
        keys = rng.integers(0, 1 << 62, n_sort, dtype=np.uint64)
        pay = rng.permutation(n_sort).astype(np.uint32)
        k, p = sort_u64(keys, pay, "device")
        order = np.argsort(keys, kind="stable")
        assert np.array_equal(k, keys[order]) and np.array_equal(p, pay[order]), n_sort
        check_lines(name, text, "device", want)
    check_tile_scan("device")


@pytest.mark.parametrize("n", pu.scan_sizes())
def test_scan_is_numpys_running_sum(n):
    check_scan(n, "device")


@pytest.mark.parametrize("n", pu.pair_sizes())
def test_scans_back_to_back(n):
    check_scan_pair(n, "device")


def test_tile_scan_is_numpys_running_sum():
    check_tile_scan("device")


def test_line_starts_of_every_short_text():
    check_short_lines("device")


@pytest.mark.parametrize("n", pu.line_sizes())
def test_line_starts_around_the_tile(n):
    check_sized_lines(n, "device")


def test_line_starts_of_64_mib():
    check_big_lines("device")


@pytest.mark.parametrize("n_cols", [256 * S, 256 * S + 1, 2 * 256 * S + 300])
def test_candidate_positions_past_one_trip_of_its_scan(n_cols):
    """cto_candidate_positions scans one count per 256 columns in place with k_scan_small: S counts are one trip, S + 1 the second, 2 S + 2
    the third.  The pack view holds what the call reads, n_cols and col_pos."""
    import torch
    from clairs_to_amd._lib import PackView
    from clairs_to_amd.extract_candidates_calling import candidate_positions
    dev = torch.device("cuda:0")
    rng = np.random.default_rng([20261026, n_cols])
    pos = np.cumsum(rng.integers(1, 4, n_cols), dtype=np.int64).astype(np.int32) + 1000
    flags = (rng.integers(0, 7, n_cols) == 0).astype(np.uint8) | ((rng.integers(0, 7, n_cols) == 0).astype(np.uint8) << 1)
    flags[-1] = 3
    lo, hi = int(pos[n_cols // 50]), int(pos[n_cols - n_cols // 70])
    d_pos, d_flags = torch.from_numpy(pos).to(dev), torch.from_numpy(flags).to(dev)
    pack = types.SimpleNamespace(device=dev, n_cols=n_cols, view=PackView(n_cols=n_cols, col_pos=d_pos.data_ptr()))
    for bit in (1, 2):
        for a, b in ((lo, hi), (1, 2 ** 31 - 1)):
            want = pos[((flags & bit) != 0) & (pos >= a) & (pos <= b)]
            counts = pu.group_sums(((flags & bit) != 0) & (pos >= a) & (pos <= b), 256 * pu.TRIP)
            assert np.all(counts[:-1] > 0) and (counts[-1] > 0 or b == hi)      # every trip of the scan carries something on; the window cuts the last
            d = pu.first_diff(candidate_positions(pack, d_flags, bit, a, b).cpu().numpy(), want)
            assert d is None, "candidate positions, %d columns, bit %d, [%d, %d]: %s" % (n_cols, bit, a, b, d)
