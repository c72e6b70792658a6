"""run_ascat (the purity/ploidy fit of the reference's Verdict chain) against what the reference wrote and printed on the same inputs
(tests/golden/ascat.json.gz, written by tests/golden/gen_ascat.py): every argv through the dispatch of `python -m clairs_to_amd`, byte for
byte, through the host path of cto_ascat_distance; the sum rule of that call against np.sum and np.nansum, bit for bit, over the lengths
at which numpy's pairwise sum changes its shape; the host path against a restatement of the reference's grid loop in numpy, on segments
freshly seeded every run."""
import os
import random
import re

import numpy as np
import pytest

import ascatsim
from conftest import ROOT, load_json_gz

SCENARIOS = ["default", "fallback", "bounds", "no_het"]
OUTPUTS = ("out_Purity_Ploidy.txt", "out_CNA.txt")
SUM_LENGTHS = list(range(1, 301)) + [511, 512, 513, 1023, 1024, 1025, 1031, 8191, 8192, 8193, 8200, 16385, 24577]


@pytest.fixture(scope="module")
def golden():
    return load_json_gz("ascat.json.gz")


def write_inputs(d, sc):
    files = ascatsim.tables(sc["spec"])
    assert ascatsim.digest(files) == sc["inputs_sha256"]
    for k, v in files.items():
        with open(os.path.join(d, k), "w") as f:
            f.write(v)


def run_scenario(sc, where, capsys):
    """the scenario's argv in the current directory: its outputs and what it printed, compared; the outputs removed"""
    from clairs_to_amd.__main__ import dispatch
    capsys.readouterr()
    dispatch("run_ascat", list(sc["argv"]) + ["--where", where])
    assert capsys.readouterr().out == sc["printed"], sc["name"]
    for fn in OUTPUTS:
        if fn not in sc["outputs"]:
            assert not os.path.exists(fn), (sc["name"], fn)
            continue
        assert open(fn).read() == sc["outputs"][fn], (sc["name"], fn)
        os.remove(fn)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


def fresh_segments(rng, n, halves=0.2, nans=0):
    """(logR, BAF, probes) of n segments: a share of BAFs at exactly 0.5, `nans` logR that are NaN"""
    s = np.column_stack((rng.normal(0, 0.4, size=n), rng.uniform(0.02, 0.5, size=n), rng.integers(1, 60, size=n).astype(float)))
    s[rng.random(n) < halves, 1] = 0.5
    if nans:
        s[rng.choice(n, size=min(nans, n), replace=False), 0] = np.nan
    return s


def restated_grid(s, gamma, psi_pos, rho_pos):
    """the grid loop of create_distance_matrix (run_ascat.py:31-60 of the reference), one cell at a time, in numpy"""
    d = np.zeros((len(psi_pos), len(rho_pos)))
    with np.errstate(invalid="ignore", over="ignore"):
        for i, psi in enumerate(psi_pos):
            for j, rho in enumerate(rho_pos):
                nA = (rho - 1 - (s[:, 1] - 1) * 2 ** (s[:, 0] / gamma) * ((1 - rho) * 2 + rho * psi)) / rho
                nB = (rho - 1 + s[:, 1] * 2 ** (s[:, 0] / gamma) * ((1 - rho) * 2 + rho * psi)) / rho
                nMinor = nA if np.nansum(nA) < np.nansum(nB) else nB
                d[i, j] = np.nansum(np.abs(nMinor - np.maximum(np.round(nMinor), 0)) ** 2 * s[:, 2] * np.where(s[:, 1] == 0.5, 0.05, 1))
    return d


def host_grid(s, gamma, psi_pos, rho_pos, stats=None):
    from clairs_to_amd.run_ascat import distance_matrix, segment_terms
    with np.errstate(invalid="ignore", over="ignore"):
        terms = segment_terms(s, gamma)
    return distance_matrix(*terms, psi_pos, rho_pos, "host", stats)


def test_run_ascat_is_a_submodule():
    from clairs_to_amd.__main__ import SUBMODULES
    assert "run_ascat" in SUBMODULES


def test_the_python_constant_is_the_header_s():
    from clairs_to_amd import run_ascat
    header = open(os.path.join(ROOT, "include", "clairsto_amd.h")).read()
    assert int(re.search(r"#define CTO_ASCAT_LDS_SEGMENTS\s+(\d+)", header).group(1)) == run_ascat.LDS_SEGMENTS


def test_the_product_does_not_import_scipy():
    assert "scipy" not in open(os.path.join(ROOT, "clairs_to_amd", "run_ascat.py")).read().split('"""', 2)[2]


def test_the_argv_is_the_reference_s_plus_where():
    """names, types and defaults of run_ascat.py:518-577, listed here as data"""
    from clairs_to_amd import run_ascat
    seen = {}
    real = run_ascat.run_ascat
    try:
        run_ascat.run_ascat = lambda *a: seen.setdefault("args", a)
        run_ascat.main([])
        assert seen.pop("args") == (None,) * 7 + (1.0, 1.5, 5.5, 0.1, 1.05, "SAMPLE", None)
        run_ascat.main(["--tumor_logr_file", "a", "--tumor_baf_file", "b", "--germline_genotypes_file", "c", "--tumor_logr_segmented_file", "d",
                        "--tumor_baf_segmented_file", "e", "--tumor_purity_ploidy_output_file", "f", "--tumor_cna_output_file", "g", "--gamma", "0.55",
                        "--min_ploidy", "1.6", "--max_ploidy", "4.8", "--min_purity", "0.2", "--max_purity", "0.9", "--sample_name", "T", "--where", "host"])
        assert seen["args"] == ("a", "b", "c", "d", "e", "f", "g", 0.55, 1.6, 4.8, 0.2, 0.9, "T", "host")
    finally:
        run_ascat.run_ascat = real


def test_the_fixture_holds_what_the_issue_asks_for(golden):
    by_name = {sc["name"]: sc for sc in golden["scenarios"]}
    assert list(by_name) == SCENARIOS
    d = by_name["default"]
    names = [c[0] for c in d["spec"]["chroms"]]
    assert len(set(names)) < len(names)                         # a chromosome name comes back
    assert d["spec"]["purity"] == 0.4 and d["seen"]["scan"] == 1 and 150 <= d["seen"]["S"] <= 400 and d["seen"]["matrix_shape"] == [100, 95]
    assert d["seen"]["far_lookups"] >= 1 and d["seen"]["merges_first_round"] >= 1 and set(d["outputs"]) == set(OUTPUTS)
    f = by_name["fallback"]
    assert f["seen"]["scan"] == 0 and f["outputs"] == {} and f["printed"].startswith("Could not find")
    b = by_name["bounds"]
    assert b["argv"][-6:] == ["--min_ploidy", "1.6", "--max_ploidy", "4.8", "--gamma", "0.55"] and b["seen"]["matrix_shape"][0] == 84
    assert set(b["outputs"]) == set(OUTPUTS)
    assert by_name["no_het"]["outputs"] == {} and by_name["no_het"]["seen"]["matrix_shape"] is None
    for sc in golden["scenarios"]:
        assert sc["seen"]["gap"] is None or sc["seen"]["gap"] >= 1e-12


@pytest.mark.parametrize("values", ["mixed", "nans", "negative_zeros"])
def test_the_sum_rule_is_numpy_s(values):
    """np.sum and np.nansum of a contiguous float64 vector, re-derived here from what numpy returns: below 8 in order, eight running
    sums up to 128, halves above, buffers of 8192"""
    from clairs_to_amd.run_ascat import nansum
    seed = random.SystemRandom().randrange(1 << 30)
    print("seed", seed)
    rng = np.random.default_rng(seed)
    for n in SUM_LENGTHS:
        if values == "negative_zeros":
            x = np.full(n, -0.0)
        else:
            x = rng.normal(0, 1, size=n) * 10.0 ** rng.integers(-8, 9, size=n)
            if values == "nans":
                x[rng.random(n) < 0.1] = np.nan
                x[rng.integers(0, n)] = np.nan
        got = nansum(x)
        assert same_bits(got, np.nansum(x)), (seed, n, values)
        if values != "nans":
            assert same_bits(got, np.sum(x)), (seed, n, values)
    assert same_bits(nansum(np.zeros(0)), 0.0)


def test_the_host_path_is_the_restated_grid_s_bits_on_the_default_grid():
    from clairs_to_amd.run_ascat import grid
    seed = random.SystemRandom().randrange(1 << 30)
    print("seed", seed)
    rng = np.random.default_rng(seed)
    n = int(rng.integers(130, 400))
    s = fresh_segments(rng, n, nans=2)
    psi_pos, rho_pos = grid(1.5, 5.5, 0.1, 1.05)
    assert (len(psi_pos), len(rho_pos)) == (100, 95)
    st = {}
    got = host_grid(s, 1.0, psi_pos, rho_pos, st)
    assert st == dict(n_cells=9500, n_segments=n, host_path=1, kernel_ms=0.0)
    want = restated_grid(s, 1.0, psi_pos, rho_pos)
    assert same_bits(got, want), (seed, n, np.argwhere(got.view(np.uint64) != want.view(np.uint64))[:5])
    assert np.isfinite(got).all() and (got > 0).all()


@pytest.mark.parametrize("case", ["one_segment", "all_half", "nan_logr", "short", "leaf_seams", "gamma", "long"])
def test_the_host_path_is_the_restated_grid_s_bits(case):
    """a part of the default grid (corners, edges, middle) at the segment counts and values that take the rules' other branches"""
    from clairs_to_amd.run_ascat import grid
    seed = random.SystemRandom().randrange(1 << 30)
    print("seed", seed)
    rng = np.random.default_rng(seed)
    psi_pos, rho_pos = grid(1.5, 5.5, 0.1, 1.05)
    psi_pos, rho_pos = np.append(psi_pos[::11], psi_pos[-1]), np.append(rho_pos[::9], rho_pos[-1])
    gamma = 0.55 if case == "gamma" else 1.0
    for n in dict(one_segment=[1], all_half=[1, 150], nan_logr=[1, 9, 140], short=[2, 7, 8, 9, 15, 16, 17], leaf_seams=[127, 128, 129, 136, 137, 257, 264],
                  gamma=[200], long=[8200])[case]:
        s = fresh_segments(rng, n, halves=1.0 if case == "all_half" else 0.2, nans=1 + n // 10 if case == "nan_logr" else 0)
        got, want = host_grid(s, gamma, psi_pos, rho_pos), restated_grid(s, gamma, psi_pos, rho_pos)
        assert same_bits(got, want), (seed, case, n)
        if case == "all_half":                                  # u = -w: the two sums are equal in every cell
            with np.errstate(invalid="ignore"):
                u = (s[:, 1] - 1) * 2 ** (s[:, 0] / gamma)
                w = s[:, 1] * 2 ** (s[:, 0] / gamma)
            assert (u == -w).all()


@pytest.mark.parametrize("name", SCENARIOS)
def test_every_scenario_byte_for_byte_on_the_host_path(golden, name, tmp_path, monkeypatch, capsys):
    sc = next(s for s in golden["scenarios"] if s["name"] == name)
    write_inputs(str(tmp_path), sc)
    monkeypatch.chdir(tmp_path)
    run_scenario(sc, "host", capsys)


def test_the_scan_that_finds_the_optimum_is_the_reference_s(golden, tmp_path, monkeypatch):
    from clairs_to_amd.run_ascat import run_ascat
    sc = golden["scenarios"][0]
    write_inputs(str(tmp_path), sc)
    monkeypatch.chdir(tmp_path)
    seen, st = {}, {}
    run_ascat("logr.txt", "baf.txt", "gg.txt", "seg_logr.txt", "seg_baf.txt", "p.txt", "c.txt", sample_name="TUM", where="host", stats=st, seen=seen)
    assert seen == dict(scan=sc["seen"]["scan"], optima=sc["seen"]["optima"])
    assert st["n_segments"] == sc["seen"]["S"] and st["n_cells"] == 9500 and st["host_path"] == 1
    assert open("p.txt").read() == sc["outputs"][OUTPUTS[0]] and open("c.txt").read() == sc["outputs"][OUTPUTS[1]]


def test_where_the_reference_dies_we_say_why():
    from clairs_to_amd.run_ascat import copy_number_segments, scan
    r_ori = np.concatenate((np.full(3, 0.1), np.full(20010, -0.2)))
    with pytest.raises(SystemExit, match="no heterozygous probe within 10000 rows"):
        copy_number_segments(0.5, 2.0, 1.0, np.array([0.4]), r_ori, np.array([20005]), len(r_ori))
    s = fresh_segments(np.random.default_rng(3), 20)
    psi_values, rho_values = np.arange(1.05, 6.05, 0.05), np.round(np.arange(0.11, 1.06, 0.01), 2)
    d = np.ones((10, 110))
    d[5, 100] = 0.5                                             # a local minimum beyond the 95 purities the scans index
    with pytest.raises(SystemExit, match="--min_purity / --max_purity are too far apart"):
        scan(d, s, 1.0, psi_values, rho_values, lambda *a: True)
    d = np.ones((110, 10))
    d[104, 5] = 0.5
    with pytest.raises(SystemExit, match="--min_ploidy / --max_ploidy are too far apart"):
        scan(d, s, 1.0, psi_values, rho_values, lambda *a: True)


def test_bad_input_is_an_error_code():
    from clairs_to_amd._lib import CtoError, check, lib
    from clairs_to_amd.run_ascat import distance_matrix
    one, psi, rho = np.ones(4), np.array([2.0, 2.5]), np.array([0.3, 0.4, 0.5])
    assert distance_matrix(one, one, one, one, psi, rho, "host").shape == (2, 3)
    empty = np.zeros(0)
    with pytest.raises(CtoError, match="0 segments"):
        distance_matrix(empty, empty, empty, empty, psi, rho, "host")
    with pytest.raises(CtoError, match="0 x 3"):
        distance_matrix(one, one, one, one, empty, rho, "host")
    with pytest.raises(CtoError, match="2 x 0"):
        distance_matrix(one, one, one, one, psi, empty, "host")
    with pytest.raises(CtoError, match="purity 1 of the grid is 0"):
        distance_matrix(one, one, one, one, psi, np.array([0.3, 0.0, 0.5]), "host")
    d = np.zeros(6)
    args = [one.ctypes.data] * 4 + [4, psi.ctypes.data, 2, rho.ctypes.data, 3, 1, d.ctypes.data, None]
    assert lib.cto_ascat_distance(*args) == 0                   # no stats: allowed
    for k in (0, 1, 2, 3, 5, 7, 10):
        bad = list(args)
        bad[k] = None
        with pytest.raises(CtoError, match="null"):
            check(lib.cto_ascat_distance(*bad))
    bad = list(args)
    bad[9] = 2
    with pytest.raises(CtoError, match="where"):
        check(lib.cto_ascat_distance(*bad))
    with pytest.raises(CtoError, match="bad arguments"):
        check(lib.cto_ascat_sum(None, 3, d.ctypes.data))
    with pytest.raises(CtoError, match="bad arguments"):
        check(lib.cto_ascat_sum(one.ctypes.data, 3, None))
    with pytest.raises(ValueError):
        distance_matrix(one, one, one, one, psi, rho, "elsewhere")
