"""aspcf with the window fits on the device (csrc/aspcf.hip) against the reference (tests/golden/aspcf.json.gz): every scenario's argv through
the dispatch of `python -m clairs_to_amd aspcf`, byte for byte; and, on windows freshly seeded every run, the kernel's costs and splits
against the host path of the same call, bit for bit, over the window lengths at which the kernel's deal of slots to threads wraps, on
exact ties, and on windows that overlap."""
import random

import numpy as np
import pytest

from conftest import load_json_gz
from test_aspcf import GAMMAS, fresh_tracks, fresh_windows, run_scenario, same_bits, write_inputs

pytestmark = pytest.mark.gpu

KMIN = 6


@pytest.fixture(scope="module")
def golden():
    return load_json_gz("aspcf.json.gz")


def both_paths(y1, y2, lo, hi, v1, v2, gamma, kmin=KMIN):
    from clairs_to_amd.aspcf import aspcf_windows
    sd, sh = {}, {}
    dev = aspcf_windows(y1, y2, lo, hi, v1, v2, kmin, gamma, "device", sd, want_cost=True)
    host = aspcf_windows(y1, y2, lo, hi, v1, v2, kmin, gamma, "host", sh, want_cost=True)
    assert sd["host_path"] == 0 and sd["kernel_ms"] > 0 and sh["host_path"] == 1
    assert sd["n_windows"] == sh["n_windows"] == len(lo) and sd["n_values"] == sh["n_values"] == len(dev[0])
    return dev, host


def assert_same(dev, host, note):
    assert (dev[0] == host[0]).all(), (note, np.nonzero(dev[0] != host[0])[0][:5])
    assert same_bits(dev[1], host[1]), (note, np.nonzero(dev[1].view(np.uint64) != host[1].view(np.uint64))[0][:5])


@pytest.mark.parametrize("name", ["default", "penalty50", "no_het"])
def test_every_scenario_byte_for_byte_on_the_device(golden, name, tmp_path, monkeypatch):
    from clairs_to_amd.aspcf import aspcf
    sc = next(s for s in golden["scenarios"] if s["name"] == name)
    write_inputs(str(tmp_path), sc)
    monkeypatch.chdir(tmp_path)
    run_scenario(sc, "device")
    if name == "default":                                       # again, for the calls' own account of where they ran
        st = {}
        aspcf("logr.txt", "baf.txt", "gg.txt", "again_LogR.txt", "again_BAF.txt", sample_name="TUM", where="device", stats=st)
        assert open("again_LogR.txt").read() == sc["outputs"]["out_LogR.txt"] and open("again_BAF.txt").read() == sc["outputs"]["out_BAF.txt"]
        assert st["host_path"] == 0 and st["kernel_ms"] > 0
        assert st["n_windows"] == sum(n >= 2 * KMIN for n in sc["seen"]["window_lengths"])


@pytest.mark.parametrize("gamma", GAMMAS)
def test_device_costs_and_splits_are_the_host_s_bits(gamma):
    """no fit, one step with one candidate, the seams of the deal of slots over 256 threads, the cap, a length drawn fresh: one call"""
    seed = random.SystemRandom().randrange(1 << 30)
    print("seed", seed)
    rng = np.random.default_rng(seed)
    lengths = [11, 12, 13] + [KMIN + 256 * j + d for j in (1, 2, 3) for d in (-1, 0, 1)] + [999, 1000, int(rng.integers(14, 1000))]
    y1, y2, lo, hi, v1, v2 = fresh_windows(rng, lengths)
    dev, host = both_paths(y1, y2, lo, hi, v1, v2, gamma)
    assert_same(dev, host, seed)
    assert not dev[0][:11].any() and not dev[1][:11].any()      # 11 values: no fit
    assert dev[0][11 + 11] == (0 if dev[1][11 + 11] < gamma else KMIN - 1)       # 12 values: the one candidate's q is below kmin, its cost gamma
    if gamma == 1e-3:
        assert (dev[0][-1000:] > 0).mean() > 0.5                # most steps split


@pytest.mark.parametrize("gamma", GAMMAS)
def test_exact_ties_take_the_host_s_index(gamma):
    """divisors of 1 and values whose sums are exact: many candidates cost exactly the same, and the first one must win"""
    rng = np.random.default_rng(7)
    constant = np.full(700, 0.25)
    blocks = np.repeat(np.where(rng.random(60) < 0.5, 0.25, 0.5), 16)[:900]
    y1 = np.concatenate((constant, blocks))
    y2 = np.concatenate((np.full(700, 0.5), np.repeat(np.where(rng.random(60) < 0.5, 0.25, 0.5), 16)[:900]))
    lo, hi = np.array([0, 700, 100]), np.array([700, 1600, 1100])
    dev, host = both_paths(y1, y2, lo, hi, np.ones(3), np.ones(3), gamma)
    assert_same(dev, host, gamma)
    if gamma == 1e-3:
        assert len(np.unique(dev[0][700:1600])) > 10            # the block window does split


@pytest.mark.parametrize("kmin", [1, 2, 9])
def test_other_shortest_segments(kmin):
    """kmin = 1: a slot is a candidate at the step after the one that finds its best[s-1] - the value must not go through a second barrier"""
    seed = random.SystemRandom().randrange(1 << 30)
    print("seed", seed)
    rng = np.random.default_rng(seed)
    lengths = [2 * kmin - 1, 2 * kmin, 2 * kmin + 1, 256 + kmin, 257 + kmin, 1000]
    y1, y2, lo, hi, v1, v2 = fresh_windows(rng, lengths)
    dev, host = both_paths(y1, y2, lo, hi, v1, v2, 1e-3, kmin)
    assert_same(dev, host, seed)
    assert (dev[0][-1000:] > 0).any()


def test_overlapping_windows_give_what_they_give_alone():
    from clairs_to_amd.aspcf import aspcf_windows
    seed = random.SystemRandom().randrange(1 << 30)
    print("seed", seed)
    rng = np.random.default_rng(seed)
    n = 2750
    y1, y2 = fresh_tracks(rng, n)
    lo = np.array([0, 701, 1502, 1750])
    hi = np.minimum(lo + 1000, n)
    v1, v2 = rng.uniform(0.05, 0.2, size=4) ** 2, rng.uniform(0.01, 0.05, size=4) ** 2
    dev, host = both_paths(y1, y2, lo, hi, v1, v2, 50)
    assert_same(dev, host, seed)
    at = 0
    for k in range(4):
        m = int(hi[k] - lo[k])
        alone = aspcf_windows(y1[lo[k]:hi[k]], y2[lo[k]:hi[k]], [0], [m], v1[k:k + 1], v2[k:k + 1], KMIN, 50, "device", want_cost=True)
        assert (alone[0] == dev[0][at:at + m]).all() and same_bits(alone[1], dev[1][at:at + m]), (seed, k)
        at += m


def test_bad_input_is_an_error_code_not_a_wrong_answer():
    from clairs_to_amd._lib import CtoError
    from clairs_to_amd.aspcf import aspcf_windows
    y1, y2 = fresh_tracks(np.random.default_rng(1), 1001)
    with pytest.raises(CtoError, match="more than 1000"):
        aspcf_windows(y1, y2, [0], [1001], [0.01], [0.01], KMIN, 50, "device")
    with pytest.raises(CtoError, match="divisors"):
        aspcf_windows(y1, y2, [0], [100], [0.0], [0.01], KMIN, 50, "device")
    bad = y1.copy()
    bad[3] = np.nan
    with pytest.raises(CtoError, match="NaN"):
        aspcf_windows(bad, y2, [0], [100], [0.01], [0.01], KMIN, 50, "device")
