"""correct_logr (the logR correction of the reference's Verdict chain) against what the reference wrote on the same inputs
(tests/golden/correct_logr.json.gz, written by tests/golden/gen_correct_logr.py), through the host path of cto_correct_logr: every argv
through the dispatch of `python -m clairs_to_amd`; keys, order, header and the three chosen columns as the reference decided them; the
residuals against the fixture's `truth` (the reference's own design and y solved in 200-bit arithmetic) within 4 x the reference's own
error, both read from the fixture; the basis at its ends and at the middle knot; the correlations against np.corrcoef on data freshly
seeded every run; what is refused."""
import os
import random
import re
from decimal import Decimal, getcontext

import numpy as np
import pytest

import correctlogrsim
from conftest import ROOT, load_json_gz

WRITING = ["default", "repeats", "constant_column", "narrow"]
SCENARIOS = WRITING + ["missing_key"]
OUTPUT = "out_LogR_Correction.txt"
getcontext().prec = 60


@pytest.fixture(scope="module")
def golden():
    return load_json_gz("correct_logr.json.gz")


def scenario(golden, name):
    return next(s for s in golden["scenarios"] if s["name"] == name)


def write_inputs(d, sc):
    files = correctlogrsim.tables(sc["spec"])
    assert correctlogrsim.digest(files) == sc["inputs_sha256"]
    for k, v in files.items():
        with open(os.path.join(d, k), "w") as f:
            f.write(v)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


def split_table(text):
    lines = text.split("\n")
    assert lines[-1] == ""
    rows = [ln.split("\t") for ln in lines[1:-1]]
    assert all(len(r) == 3 for r in rows)
    return lines[0], [tuple(r[:2]) for r in rows], [r[2] for r in rows]


def max_error(values, truth):
    """max |value - truth|, the values taken exactly, the truth as the fixture's decimal strings"""
    assert len(values) == len(truth)
    return max(abs(Decimal(float(v)) - Decimal(t)) for v, t in zip(values, truth))


def check_against_reference(sc, text, stats):
    """what the reference decided, and the accuracy condition; prints the ratio it measures"""
    header, keys, values = split_table(text)
    ref_header, ref_keys, _ = split_table(sc["output"])
    assert header == ref_header == "Chromosome\tPosition\tTUM" and keys == ref_keys
    assert [stats["col_insert"], stats["col_amplic"], stats["col_replic"]] == sc["seen"]["cols"]
    assert stats["n_rows"] == sc["seen"]["rows"] and stats["n_gc"] == sc["spec"]["G"] and stats["n_rt"] == sc["spec"]["T"]
    err, ref_err = max_error([float(v) for v in values], sc["seen"]["truth"]), Decimal(sc["seen"]["ref_err"])
    print(sc["name"], "max |ours - truth| = %.3g, the reference's = %.3g, ratio %.2f" % (err, ref_err, err / ref_err))
    assert err <= 4 * ref_err, (sc["name"], float(err), float(ref_err))


def fresh_tables(rng, n, g, t):
    """logR, GC and RT tables whose columns all carry some of two latent tracks: no window's choice is forced"""
    a, b = rng.uniform(0.2, 0.8, size=n), rng.normal(0, 1, size=n)
    gc = rng.uniform(0.1, 0.9, size=(1, g)) * a[:, None] + rng.uniform(0, 0.3, size=(n, g))
    rt = 40 + rng.uniform(5, 20, size=(1, t)) * b[:, None] + rng.normal(0, 6, size=(n, t))
    logr = -1.5 * (a - 0.5) + 4 * (a - 0.5) ** 2 + 0.05 * b + rng.normal(0, 0.1, size=n)
    return logr, gc, rt


def restated_basis(x, lo, hi):
    """de Boor's recurrence on the knots lo x 4, the middle, hi x 4, as csrc/correctlogr.hip states it (rule 2); lo < hi"""
    mid = (hi - lo) / 2.0 + lo
    t = [lo] * 4 + [mid] + [hi] * 4
    out = np.zeros((len(x), 5))
    for i, xv in enumerate(x):
        ell = 3 if xv < mid else 4
        h = [1.0, 0.0, 0.0, 0.0]
        for j in range(1, 4):
            hh = h[:j]
            h[0] = 0.0
            for n in range(1, j + 1):
                xb, xa = t[ell + n], t[ell + n - j]
                w = hh[n - 1] / (xb - xa)
                h[n - 1] += w * (xb - xv)
                h[n] = w * (xv - xa)
        out[i, ell - 3:ell + 1] = h
        if xv == lo or xv == hi:                                # the ends are exact
            out[i] = [float(xv == lo), 0.0, 0.0, 0.0, float(xv == hi)]
    return out


def restated_corr(table, logr):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.abs(np.corrcoef(table, logr, rowvar=False))[0, 1:]


def test_correct_logr_is_a_submodule():
    from clairs_to_amd.__main__ import SUBMODULES
    assert "correct_logr" in SUBMODULES


def test_the_python_constant_is_the_header_s():
    from clairs_to_amd import correct_logr
    header = open(os.path.join(ROOT, "include", "clairsto_amd.h")).read()
    assert int(re.search(r"#define CTO_CORRECT_LOGR_BLOCK_ROWS\s+(\d+)", header).group(1)) == correct_logr.BLOCK_ROWS


def test_the_package_imports_neither_scipy_nor_scikit_learn():
    pkg = os.path.join(ROOT, "clairs_to_amd")
    for fn in sorted(os.listdir(pkg)):
        if fn.endswith(".py"):
            assert not re.search(r"^\s*(import|from)\s+(scipy|sklearn)\b", open(os.path.join(pkg, fn)).read(), re.M), fn


def test_the_argv_is_the_reference_s_plus_where():
    """names, types and defaults of correct_logr.py:96-121, listed here as data"""
    from clairs_to_amd import correct_logr
    seen = {}
    real = correct_logr.correct_logr
    try:
        correct_logr.correct_logr = lambda *a: seen.setdefault("args", a)
        correct_logr.main([])
        assert seen.pop("args") == (None, None, None, None, "SAMPLE", None)
        correct_logr.main(["--tumor_logr_file", "a", "--gc_content_file", "b", "--replication_timing_file", "c", "--tumor_logr_correction_output_file", "d",
                           "--sample_name", "T", "--where", "host"])
        assert seen["args"] == ("a", "b", "c", "d", "T", "host")
    finally:
        correct_logr.correct_logr = real


def test_the_fixture_holds_what_the_issue_asks_for(golden):
    by_name = {sc["name"]: sc for sc in golden["scenarios"]}
    assert list(by_name) == SCENARIOS
    d = by_name["default"]
    assert 2500 <= d["seen"]["rows"] <= 3500 and d["spec"]["G"] == 18 and d["spec"]["T"] == 12 and d["spec"]["shuffle"] and d["spec"]["extra"] > 0
    assert len({c[0] for c in d["spec"]["chroms"]}) >= 3
    assert by_name["repeats"]["spec"]["repeats"] > 0
    c = by_name["constant_column"]
    assert c["spec"]["constant_gc"] == 3 and c["seen"]["corr_gc"][2] == "nan" and c["seen"]["cols"][0] == 2
    n = by_name["narrow"]
    assert (n["spec"]["G"], n["spec"]["T"]) == (8, 1) and n["seen"]["cols"][1:] == [7, 0]
    m = by_name["missing_key"]
    assert m["returncode"] != 0 and m["output"] is None and m["error"].startswith("KeyError")
    for name in WRITING:
        sc = by_name[name]
        assert sc["returncode"] == 0 and sc["seen"]["rank"] == 12 and len(sc["seen"]["truth"]) == sc["seen"]["rows"]
        assert all(g is None or g >= 1e-6 for g in sc["seen"]["gaps"])
        assert 0 < float(sc["seen"]["ref_err"]) < 1e-14
        again = max_error([float(v) for v in split_table(sc["output"])[2]], sc["seen"]["truth"])     # ref_err is what it says it is
        assert abs(again / Decimal(sc["seen"]["ref_err"]) - 1) < Decimal("1e-6")


@pytest.mark.parametrize("name", WRITING)
def test_every_scenario_on_the_host_path(golden, name, tmp_path, monkeypatch):
    from clairs_to_amd.__main__ import dispatch
    from clairs_to_amd.correct_logr import correct_logr
    sc = scenario(golden, name)
    write_inputs(str(tmp_path), sc)
    monkeypatch.chdir(tmp_path)
    dispatch("correct_logr", list(sc["argv"]) + ["--where", "host"])
    text = open(OUTPUT).read()
    st = {}
    correct_logr("logr.txt", "gc.txt", "rt.txt", "again.txt", "TUM", "host", st)          # the function form, for the call's own account
    assert open("again.txt").read() == text and st["host_path"] == 1 and st["kernel_ms"] == 0.0
    check_against_reference(sc, text, st)


def test_a_missing_key_is_named_and_nothing_is_written(golden, tmp_path, monkeypatch):
    from clairs_to_amd.__main__ import dispatch
    sc = scenario(golden, "missing_key")
    write_inputs(str(tmp_path), sc)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        dispatch("correct_logr", list(sc["argv"]) + ["--where", "host"])
    assert e.value.code not in (0, None) and repr(tuple(sc["missing"])) in str(e.value.code) and "GC content" in str(e.value.code)
    assert repr(tuple(sc["missing"])) in sc["error"]
    assert not os.path.exists(OUTPUT)


def test_seven_gc_columns_are_refused(golden, tmp_path, monkeypatch):
    from clairs_to_amd._lib import CtoError
    from clairs_to_amd.__main__ import dispatch
    from clairs_to_amd.correct_logr import fit
    rng = np.random.default_rng(5)
    logr, gc, rt = fresh_tables(rng, 300, 7, 3)
    with pytest.raises(CtoError, match="7 GC columns"):
        fit(logr, gc, rt, "host")
    sc = scenario(golden, "narrow")
    files = correctlogrsim.tables(dict(sc["spec"], G=7))
    monkeypatch.chdir(tmp_path)
    for k, v in files.items():
        open(k, "w").write(v)
    with pytest.raises(SystemExit, match="7 value columns"):
        dispatch("correct_logr", list(sc["argv"]) + ["--where", "host"])
    assert not os.path.exists(OUTPUT)


def test_the_output_is_a_logr_table_for_the_later_steps(golden, tmp_path, monkeypatch):
    from clairs_to_amd.__main__ import dispatch
    from clairs_to_amd.aspcf import finite_column
    from clairs_to_amd.predict_germline_genotypes import read_table
    sc = scenario(golden, "repeats")
    write_inputs(str(tmp_path), sc)
    monkeypatch.chdir(tmp_path)
    dispatch("correct_logr", list(sc["argv"]) + ["--where", "host"])
    table, before = read_table(OUTPUT), read_table("logr.txt")
    assert list(table) == list(before) and len(table) == sc["seen"]["rows"]
    v = finite_column(table, "logR")                            # as aspcf takes its --tumor_logr_file
    assert v.shape == (len(table),) and [str(x) for x in v] == list(table.values())


def test_the_basis_at_its_ends_and_at_the_middle_knot():
    from clairs_to_amd.correct_logr import bspline_basis
    seed = random.SystemRandom().randrange(1 << 30)
    print("seed", seed)
    rng = np.random.default_rng(seed)
    for lo, hi in [(0.0, 1.0), (0.214, 0.713), (-3.5, 80.25), tuple(np.sort(rng.normal(0, 10, size=2)))]:
        mid = (hi - lo) / 2.0 + lo
        below, above = np.nextafter(mid, lo), np.nextafter(mid, hi)
        x = np.concatenate(([lo, hi, mid, below, above], rng.uniform(lo, hi, size=500)))
        x = np.minimum(np.maximum(x, lo), hi)
        got = bspline_basis(x, lo, hi)
        assert same_bits(got[0], [1.0, 0.0, 0.0, 0.0, 0.0]) and same_bits(got[1], [0.0, 0.0, 0.0, 0.0, 1.0]), (seed, lo, hi)
        assert same_bits(got, restated_basis(x, lo, hi)), (seed, lo, hi)                  # mid takes the right interval there
        assert got[2, 0] == 0.0 and got[2, 4] == 0.0 and got[3, 0] > 0.0 and got[3, 4] == 0.0 and got[4, 0] == 0.0 and got[4, 4] > 0.0
        assert (got >= 0).all() and np.abs(got.sum(axis=1) - 1).max() <= 4 * np.finfo(float).eps


@pytest.mark.parametrize("shape", [(2000, 18, 12), (300, 8, 1), (777, 13, 16)])
def test_the_correlations_are_numpy_s(shape):
    from clairs_to_amd.correct_logr import chosen_columns, fit
    seed = random.SystemRandom().randrange(1 << 30)
    print("seed", seed)
    rng = np.random.default_rng(seed)
    n, g, t = shape
    logr, gc, rt = fresh_tables(rng, n, g, t)
    gc[:, 6] = 0.25                                              # constant, never chosen (entry 5 is NaN and wins: column 5 is chosen)
    if t > 1:
        rt[:, t - 1] = -2.0
    st = {}
    corr_gc, corr_rt, residual = fit(logr, gc, rt, "host", st)
    want_gc, want_rt = restated_corr(gc, logr), restated_corr(rt, logr)
    for got, want in ((corr_gc, want_gc), (corr_rt, want_rt)):
        assert got.shape == want.shape and (np.isnan(got) == np.isnan(want)).all(), seed
        assert np.nanmax(np.abs(got - want)) <= 1e-12, seed
    assert np.isnan(corr_gc[5]) and st["col_insert"] == 5 and (t == 1 or (np.isnan(corr_rt[t - 2]) and st["col_replic"] == t - 2))
    assert (st["col_insert"], st["col_amplic"], st["col_replic"]) == chosen_columns(want_gc, want_rt) == chosen_columns(corr_gc, corr_rt)
    assert np.isfinite(residual).all() and abs(residual.sum()) < 1e-9 and residual.std() < logr.std()


def test_bad_input_is_an_error_code():
    from clairs_to_amd._lib import CtoError, check, lib
    from clairs_to_amd.correct_logr import fit
    rng = np.random.default_rng(11)
    logr, gc, rt = fresh_tables(rng, 400, 9, 2)
    assert fit(logr, gc, rt, "host")[2].shape == (400,)
    with pytest.raises(CtoError, match="1 rows"):
        fit(logr[:1], gc[:1], rt[:1], "host")
    with pytest.raises(CtoError, match="0 replication-timing columns"):
        fit(logr, gc, rt[:, :0], "host")
    for bad in (np.inf, -np.inf, np.nan):
        for which in range(3):
            tables = [logr.copy(), gc.copy(), rt.copy()]
            tables[which][(123,) if which == 0 else (123, 1)] = bad
            with pytest.raises(CtoError, match="not finite"):
                fit(*tables, "host")
    flat = gc.copy()
    flat[:, 0] = 0.5                                            # every correlation NaN: column 0 is chosen, and it is constant
    with pytest.raises(CtoError, match="column 0 of the GC table, chosen for the fit, is constant"):
        fit(logr, flat, rt, "host")
    two = gc.copy()
    two[:, 3] = two[:, 0]                                        # entry 2 of the row is 1: column 2 is chosen
    two[:, 2] = np.where(rng.random(400) < 0.5, 0.1, 0.9)        # ... and it takes two values only: two of its four functions are zero
    st = {}
    with pytest.raises(CtoError, match="pivot . of the Cholesky factor is not positive: GC column 2"):
        fit(logr, two, rt, "host", st)
    assert st["col_insert"] == 2
    corr, res = np.zeros(9), np.zeros(400)
    args = [logr.ctypes.data, 400, gc.ctypes.data, 9, rt.ctypes.data, 2, 1, corr.ctypes.data, corr.ctypes.data, res.ctypes.data, None]
    assert lib.cto_correct_logr(*args) == 0                     # no stats: allowed
    for k in (0, 2, 4, 7, 8, 9):
        bad = list(args)
        bad[k] = None
        with pytest.raises(CtoError, match="null"):
            check(lib.cto_correct_logr(*bad))
    bad = list(args)
    bad[6] = 2
    with pytest.raises(CtoError, match="where"):
        check(lib.cto_correct_logr(*bad))
    with pytest.raises(CtoError, match="empty"):
        check(lib.cto_correct_logr_basis(logr.ctypes.data, 3, 1.0, 1.0, res.ctypes.data))
    with pytest.raises(ValueError):
        fit(logr, gc, rt, "elsewhere")
    with pytest.raises(ValueError):
        fit(logr, gc[:-1], rt, "host")
