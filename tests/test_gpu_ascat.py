"""run_ascat with the grid on the device (csrc/ascat.hip) against the reference (tests/golden/ascat.json.gz): every scenario's argv through
the dispatch of `python -m clairs_to_amd run_ascat`, byte for byte; and, on segments freshly seeded every run, the kernel's whole matrix
against the host path of the same call, bit for bit, over the segment counts at which the pairwise sum changes its shape, on both sides
of the buffers of 8192 and of what LDS holds, on values that are not finite, and on grids that do not fill the last workgroup."""
import random

import numpy as np
import pytest

from conftest import load_json_gz
from test_ascat import OUTPUTS, SCENARIOS, fresh_segments, run_scenario, same_bits, write_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load_json_gz("ascat.json.gz")


def default_grid():
    from clairs_to_amd.run_ascat import grid
    psi_pos, rho_pos = grid(1.5, 5.5, 0.1, 1.05)
    assert (len(psi_pos), len(rho_pos)) == (100, 95)
    return psi_pos, rho_pos


def small_grid():
    psi_pos, rho_pos = default_grid()
    return psi_pos[::24], rho_pos[::15]                         # 5 x 7, the corners of the default grid's low ends included


def both_paths(u, w, cnt, wgt, psi_pos, rho_pos, note):
    from clairs_to_amd.run_ascat import distance_matrix
    sd, sh = {}, {}
    dev = distance_matrix(u, w, cnt, wgt, psi_pos, rho_pos, "device", sd)
    host = distance_matrix(u, w, cnt, wgt, psi_pos, rho_pos, "host", sh)
    assert sd["host_path"] == 0 and sd["kernel_ms"] > 0 and sh["host_path"] == 1
    assert sd["n_cells"] == sh["n_cells"] == len(psi_pos) * len(rho_pos) and sd["n_segments"] == sh["n_segments"] == len(u)
    assert same_bits(dev, host), (note, len(u), np.argwhere(dev.view(np.uint64) != host.view(np.uint64))[:5])
    return dev


def terms_of(s, gamma=1.0):
    from clairs_to_amd.run_ascat import segment_terms
    with np.errstate(invalid="ignore", over="ignore"):
        return segment_terms(s, gamma)


@pytest.mark.parametrize("name", SCENARIOS)
def test_every_scenario_byte_for_byte_on_the_device(golden, name, tmp_path, monkeypatch, capsys):
    from clairs_to_amd.run_ascat import run_ascat
    sc = next(s for s in golden["scenarios"] if s["name"] == name)
    write_inputs(str(tmp_path), sc)
    monkeypatch.chdir(tmp_path)
    run_scenario(sc, "device", capsys)
    if sc["seen"]["matrix_shape"]:                              # again, for the call's own account of where it ran
        st = {}
        extra = dict(zip(("min_ploidy", "max_ploidy", "gamma"), (1.6, 4.8, 0.55))) if name == "bounds" else {}
        run_ascat("logr.txt", "baf.txt", "gg.txt", "seg_logr.txt", "seg_baf.txt", "p.txt", "c.txt", sample_name="TUM", where="device", stats=st, **extra)
        assert st["host_path"] == 0 and st["kernel_ms"] > 0
        assert st["n_segments"] == sc["seen"]["S"] and st["n_cells"] == sc["seen"]["matrix_shape"][0] * sc["seen"]["matrix_shape"][1]
        if sc["outputs"]:
            assert open("p.txt").read() == sc["outputs"][OUTPUTS[0]] and open("c.txt").read() == sc["outputs"][OUTPUTS[1]]


@pytest.mark.parametrize("n", [1, 7, 8, 9, 127, 128, 129, 136, 137, 257, 264, "fresh"])
def test_the_default_grid_is_the_host_s_bits(n):
    seed = random.SystemRandom().randrange(1 << 30)
    print("seed", seed)
    rng = np.random.default_rng(seed)
    if n == "fresh":
        n = int(rng.integers(130, 2001))
        print("segments", n)
    d = both_paths(*terms_of(fresh_segments(rng, n, nans=n // 50)), *default_grid(), seed)
    assert np.isfinite(d).all() and (d >= 0).all() and d.max() > 0


@pytest.mark.parametrize("n", [8191, 8192, 8193, 8200, 16385])
def test_the_buffers_of_8192_and_the_global_memory_path(n):
    seed = random.SystemRandom().randrange(1 << 30)
    print("seed", seed)
    both_paths(*terms_of(fresh_segments(np.random.default_rng(seed), n, nans=3)), *small_grid(), seed)


@pytest.mark.parametrize("delta", [0, 1])
def test_the_last_count_that_fits_lds_and_the_first_that_does_not(delta):
    from clairs_to_amd.run_ascat import LDS_SEGMENTS
    seed = random.SystemRandom().randrange(1 << 30)
    print("seed", seed)
    both_paths(*terms_of(fresh_segments(np.random.default_rng(seed), LDS_SEGMENTS + delta)), *small_grid(), seed)


@pytest.mark.parametrize("case", ["not_finite", "every_weight_small", "equal_sums"])
def test_values_that_take_the_other_branches(case):
    seed = random.SystemRandom().randrange(1 << 30)
    print("seed", seed)
    rng = np.random.default_rng(seed)
    n = 300
    u, w, cnt, wgt = terms_of(fresh_segments(rng, n))
    u, w, wgt = u.copy(), w.copy(), wgt.copy()
    if case == "not_finite":
        for arr in (u, w):
            at = rng.choice(n, size=9, replace=False)
            arr[at[:3]], arr[at[3:6]], arr[at[6:]] = np.nan, np.inf, -np.inf
    elif case == "every_weight_small":
        wgt[:] = 0.05
    else:
        u = -w                                                  # nA == nB in every cell: the sums are equal and nB is taken
    d = both_paths(u, w, cnt, wgt, *default_grid(), (seed, case))
    if case == "equal_sums":
        assert same_bits(d, both_paths(-2 * w, w, cnt, wgt, *default_grid(), (seed, case)))     # nA is larger now: nB again
    if case == "not_finite":
        assert not np.isnan(d).any()


@pytest.mark.parametrize("shape", [(1, 1), (1, 95), (100, 1), (3, 11), (7, 9)])
def test_other_grids(shape):
    """one cell, one row, one column, 33 cells (one more than a workgroup's 32) and 63"""
    seed = random.SystemRandom().randrange(1 << 30)
    print("seed", seed)
    rng = np.random.default_rng(seed)
    psi_pos, rho_pos = default_grid()
    psi_pos, rho_pos = rng.choice(psi_pos, size=shape[0], replace=False), rng.choice(rho_pos, size=shape[1], replace=False)
    d = both_paths(*terms_of(fresh_segments(rng, 200)), psi_pos, rho_pos, seed)
    assert d.shape == shape


def test_bad_input_is_an_error_code_on_the_device_path():
    from clairs_to_amd._lib import CtoError
    from clairs_to_amd.run_ascat import distance_matrix
    one, psi, rho, empty = np.ones(4), np.array([2.0, 2.5]), np.array([0.3, 0.4, 0.5]), np.zeros(0)
    with pytest.raises(CtoError, match="0 segments"):
        distance_matrix(empty, empty, empty, empty, psi, rho, "device")
    with pytest.raises(CtoError, match="0 x 3"):
        distance_matrix(one, one, one, one, empty, rho, "device")
    with pytest.raises(CtoError, match="2 x 0"):
        distance_matrix(one, one, one, one, psi, empty, "device")
    with pytest.raises(CtoError, match="purity 2 of the grid is 0"):
        distance_matrix(one, one, one, one, psi, np.array([0.3, 0.4, 0.0]), "device")
    assert distance_matrix(one, one, one, one, psi, rho, "device").shape == (2, 3)
