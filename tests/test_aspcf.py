"""aspcf (the segmentation step of the reference's Verdict chain) against what the reference wrote on the same inputs
(tests/golden/aspcf.json.gz, written by tests/golden/gen_aspcf.py): every argv through the dispatch of `python -m clairs_to_amd`, byte for
byte (digest for digest where the fixture stores digests), through the host path of cto_aspcf_windows; that path's costs and splits, on
windows freshly seeded every run, against a short restatement of the recurrence's rules with Python's scalar ** 2 as the square; the
prepared squares against Python's; the running median against scipy's; the single-track recurrence against its restatement."""
import hashlib
import os
import random

import numpy as np
import pytest

import aspcfsim
from conftest import load_json_gz

GAMMAS = [1000, 50, 1e-3]


@pytest.fixture(scope="module")
def golden():
    return load_json_gz("aspcf.json.gz")


def write_inputs(d, sc):
    files = aspcfsim.tables(sc["spec"])
    assert aspcfsim.digest(files) == sc["inputs_sha256"]
    for k, v in files.items():
        with open(os.path.join(d, k), "w") as f:
            f.write(v)


def run_scenario(sc, where):
    """the scenario's argv in the current directory, its outputs compared and removed"""
    from clairs_to_amd.__main__ import dispatch
    dispatch("aspcf", list(sc["argv"]) + ["--where", where])
    for fn in ("out_LogR.txt", "out_BAF.txt"):
        if fn not in sc["outputs"]:
            assert not os.path.exists(fn), (sc["name"], fn)
            continue
        got = open(fn).read()
        if sc["store"] == "sha256":
            got = hashlib.sha256(got.encode()).hexdigest()
        assert got == sc["outputs"][fn], (sc["name"], fn)
        os.remove(fn)


def same_bits(a, b):
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


def sq(x):
    return float(x) ** 2                                        # Python's float power: libm's pow


def restated_window(a, b, v1, v2, kmin, gamma):
    """the rules of the two-track recurrence for one window -> (best_cost, best_split)"""
    N = len(a)
    best, split = np.zeros(N), np.zeros(N, dtype=np.int32)
    if N < 2 * kmin:
        return best, split
    a, b, v1, v2 = [float(v) for v in a], [float(v) for v in b], float(v1), float(v2)
    i1 = i2 = q1 = q2 = 0.0
    for i in range(kmin):
        i1 += a[i]
        q1 += a[i] * a[i]
        i2 += b[i]
        q2 += b[i] * b[i]
    best[kmin - 1] = (q1 - i1 * (i1 / kmin)) / v1 + (q2 - i2 * (i2 / kmin)) / v2
    S1, K1, S2, K2 = np.zeros(N), np.zeros(N), np.zeros(N), np.zeros(N)
    for n in range(kmin + 1, N + 1):
        S1[kmin:n] += a[n - 1]
        K1[kmin:n] += sq(a[n - 1])
        S2[kmin:n] += b[n - 1]
        K2[kmin:n] += sq(b[n - 1])
        t1, t2 = (float(S1[kmin]) + i1) / n, (float(S2[kmin]) + i2) / n
        tot = ((float(K1[kmin]) + q1) - n * sq(t1)) / v1 + ((float(K2[kmin]) + q2) - n * sq(t2)) / v2
        if n < 2 * kmin:
            best[n - 1] = tot
            continue
        s = np.arange(kmin, n - kmin + 1)
        c = (best[s - 1] + (K1[s] - S1[s] * (S1[s] / (n - s))) / v1) + (K2[s] - S2[s] * (S2[s] / (n - s))) / v2
        q = kmin + int(np.argmin(c)) - 1
        cost = (float(c[q - kmin]) if q >= kmin else 0.0) + gamma
        if tot < cost:
            q, cost = 0, tot
        best[n - 1], split[n - 1] = cost, q
    return best, split


def restated_exact_pcf(y, kmin, gamma):
    """the rules of the single-track recurrence -> yhat"""
    N = len(y)
    y = [float(v) for v in y]
    i0 = q0 = 0.0
    for i in range(kmin):
        i0 += y[i]
        q0 += y[i] * y[i]
    best, aver, split = np.zeros(N), np.zeros(N), np.zeros(N, dtype=int)
    aver[kmin - 1] = i0 / kmin
    best[kmin - 1] = q0 - i0 * (i0 / kmin)
    S, K = np.zeros(N), np.zeros(N)
    for n in range(kmin + 1, N + 1):
        S[kmin:n] += y[n - 1]
        K[kmin:n] += sq(y[n - 1])
        t_aver = (float(S[kmin]) + i0) / n
        t_cost = (float(K[kmin]) + q0) - n * sq(t_aver)
        if n < 2 * kmin:
            aver[n - 1], best[n - 1] = t_aver, t_cost
            continue
        s = np.arange(kmin, n - kmin + 1)
        c = ((best[s - 1] + K[s]) - S[s] * (S[s] / (n - s))) + gamma
        q = kmin + int(np.argmin(c)) - 1
        cost, av = (float(c[q - kmin]), float(S[q]) / (n - q)) if q >= kmin else (0.0, 0.0)
        if t_cost < cost:
            q, cost, av = 0, t_cost, t_aver
        best[n - 1], aver[n - 1], split[n - 1] = cost, av, q
    yhat = np.zeros(N)
    n = N
    while n > 0:
        yhat[split[n - 1]:n] = aver[n - 1]
        n = split[n - 1]
    return yhat


def fresh_tracks(rng, n):
    """a logR-like and a flipped-BAF-like track of n values: levels of 5 - 60 values with noise"""
    y1, y2 = np.empty(n), np.empty(n)
    i = 0
    while i < n:
        m = int(rng.integers(5, 61))
        y1[i:i + m] = rng.uniform(-0.8, 0.8) + rng.normal(0, 0.1, size=len(y1[i:i + m]))
        y2[i:i + m] = np.clip(0.5 - rng.uniform(0, 0.3) + rng.normal(0, 0.03, size=len(y2[i:i + m])), 0.01, 0.5)
        i += m
    return y1, y2


def fresh_windows(rng, lengths):
    """windows of the given lengths, one after the other in one pair of arrays, and divisors as a MAD squared would be"""
    y1, y2 = fresh_tracks(rng, int(sum(lengths)))
    hi = np.cumsum(lengths).astype(np.int64)
    return y1, y2, hi - np.asarray(lengths, dtype=np.int64), hi, rng.uniform(0.05, 0.2, size=len(lengths)) ** 2, rng.uniform(0.01, 0.05, size=len(lengths)) ** 2


def restated_call(y1, y2, lo, hi, v1, v2, kmin, gamma):
    parts = [restated_window(y1[a:b], y2[a:b], p, q, kmin, gamma) for a, b, p, q in zip(lo, hi, v1, v2)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def test_aspcf_is_a_submodule():
    from clairs_to_amd.__main__ import SUBMODULES
    assert "aspcf" in SUBMODULES


def test_the_python_constant_is_the_header_s():
    import re
    from clairs_to_amd import aspcf
    from conftest import ROOT
    header = open(os.path.join(ROOT, "include", "clairsto_amd.h")).read()
    assert int(re.search(r"#define CTO_ASPCF_MAX_WINDOW\s+(\d+)", header).group(1)) == aspcf.MAX_WINDOW == 1000


def test_the_product_does_not_import_scipy():
    from conftest import ROOT
    assert "scipy" not in open(os.path.join(ROOT, "clairs_to_amd", "aspcf.py")).read().split('"""', 2)[2]


def test_the_fixture_holds_what_the_issue_asks_for(golden):
    by_name = {sc["name"]: sc for sc in golden["scenarios"]}
    assert list(by_name) == ["default", "penalty50", "no_het"]
    d = by_name["default"]
    hets = [c[1] for c in d["spec"]["chroms"]]
    assert {0, 1, 5, 6, 11, 12, 13, 899, 900, 901, 1100, 2600} <= set(hets)
    names = [c[0] for c in d["spec"]["chroms"]]
    assert len(set(names)) < len(names)                         # a chromosome name comes back
    assert d["seen"]["gammas"] == [1000] and d["seen"]["replaced"] > 5 and d["seen"]["window_lengths"].count(1000) >= 2
    assert "--penalty" not in d["argv"]
    p = by_name["penalty50"]
    assert p["argv"][-2:] == ["--penalty", "50"] and p["seen"]["gammas"][:2] == [50, 70]
    assert by_name["no_het"]["outputs"] == {}
    for sc in golden["scenarios"]:
        assert sc["seen"]["argmin_ties"] == 0
        assert sc["seen"]["argmin_gap"] is None or sc["seen"]["argmin_gap"] >= 1e-12


@pytest.mark.parametrize("name", ["default", "penalty50", "no_het"])
def test_every_scenario_byte_for_byte_on_the_host_path(golden, name, tmp_path, monkeypatch):
    sc = next(s for s in golden["scenarios"] if s["name"] == name)
    write_inputs(str(tmp_path), sc)
    monkeypatch.chdir(tmp_path)
    run_scenario(sc, "host")


def test_a_logr_that_is_not_finite_is_refused_by_name(golden, tmp_path, monkeypatch):
    from clairs_to_amd.__main__ import dispatch
    sc = golden["scenarios"][2]
    files = aspcfsim.tables(dict(sc["spec"], chroms=[("chr1", 20, 300)]))
    rows = files["logr.txt"].split("\n")
    ctg, pos, _ = rows[8].split("\t")
    rows[8] = "%s\t%s\tnan" % (ctg, pos)
    files["logr.txt"] = "\n".join(rows)
    for k, v in files.items():
        (tmp_path / k).write_text(v)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        dispatch("aspcf", list(sc["argv"]) + ["--where", "host"])
    assert "%s:%s" % (ctg, pos) in str(e.value) and "logR" in str(e.value)
    assert not os.path.exists("out_LogR.txt") and not os.path.exists("out_BAF.txt")


@pytest.mark.parametrize("gamma", GAMMAS)
def test_host_costs_and_splits_are_the_restated_rules_bits(gamma):
    from clairs_to_amd.aspcf import aspcf_windows
    seed = random.SystemRandom().randrange(1 << 30)
    print("seed", seed)
    rng = np.random.default_rng(seed)
    lengths = [11, 12, 13, 64, 261, 262, 263, 1000]
    y1, y2, lo, hi, v1, v2 = fresh_windows(rng, lengths)
    st = {}
    split, cost = aspcf_windows(y1, y2, lo, hi, v1, v2, 6, gamma, "host", st, want_cost=True)
    assert st == dict(n_windows=len(lengths), n_values=sum(lengths), host_path=1, kernel_ms=0.0)
    want_cost, want_split = restated_call(y1, y2, lo, hi, v1, v2, 6, gamma)
    assert (split == want_split).all(), (seed, np.nonzero(split != want_split)[0][:5])
    assert same_bits(cost, want_cost), (seed, np.nonzero(cost.view(np.uint64) != want_cost.view(np.uint64))[0][:5])
    assert not split[:11].any() and not cost[:11].any()         # 11 values: no fit
    if gamma == 1e-3:
        assert (split[-1000:][12:] > 0).mean() > 0.5            # most steps split
    assert (aspcf_windows(y1, y2, lo, hi, v1, v2, 6, gamma, "host") == split).all()        # without best_cost


@pytest.mark.parametrize("kmin", [1, 2, 7])
def test_other_shortest_segments_on_the_host_path(kmin):
    from clairs_to_amd.aspcf import aspcf_windows
    seed = random.SystemRandom().randrange(1 << 30)
    print("seed", seed)
    lengths = [2 * kmin - 1, 2 * kmin, 2 * kmin + 1, 150]
    y1, y2, lo, hi, v1, v2 = fresh_windows(np.random.default_rng(seed), lengths)
    split, cost = aspcf_windows(y1, y2, lo, hi, v1, v2, kmin, 1e-3, "host", want_cost=True)
    want_cost, want_split = restated_call(y1, y2, lo, hi, v1, v2, kmin, 1e-3)
    assert (split == want_split).all() and same_bits(cost, want_cost), seed


def test_the_prepared_squares_are_python_s():
    """the host code squares with libm's pow, which is what `v ** 2` of a Python float (and of a numpy scalar) calls: not always v * v"""
    import ctypes as C  # noqa: F401
    from clairs_to_amd._lib import check, lib
    rng = np.random.default_rng(12)
    x = np.concatenate((rng.normal(0, 0.5, size=60000), rng.uniform(0, 0.5, size=40000)))
    out = np.empty_like(x)
    check(lib.cto_aspcf_squares(x.ctypes.data, len(x), out.ctypes.data))
    want = np.array([float(v) ** 2 for v in x])
    assert same_bits(out, want)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 50, 51, 52, 53, 1000])
def test_running_median_is_scipy_s(n):
    ndimage = pytest.importorskip("scipy.ndimage")
    from clairs_to_amd.aspcf import running_median
    rng = np.random.default_rng(100 + n)
    x = np.round(rng.normal(0, 1, size=n), 1) + 0.0             # rounded: equal values occur (+ 0.0: no -0.0, which equals 0.0 with other bits)
    k = 25
    width = 2 * k + 1
    if width > n:
        width = 1 if n == 0 else n - 1 if n % 2 == 0 else n
    got = running_median(x, k)
    want = ndimage.median_filter(x, size=width, mode="reflect")
    assert same_bits(got, np.asarray(want, dtype=np.float64))


@pytest.mark.parametrize("gamma", [250, 12])
@pytest.mark.parametrize("n", [11, 12, 13, 300])
def test_exact_pcf_is_its_restated_rules_bits(n, gamma):
    from clairs_to_amd.aspcf import exact_pcf
    seed = random.SystemRandom().randrange(1 << 30)
    print("seed", seed)
    y = 4 * fresh_tracks(np.random.default_rng(seed), n)[0]     # levels far enough apart for the smaller penalty to split
    got = exact_pcf(y, 6, gamma)
    want = np.full(n, np.mean(y)) if n < 12 else restated_exact_pcf(y, 6, gamma)
    assert same_bits(got, want), seed
    if n == 300 and gamma == 12:
        assert len(np.unique(got)) > 2


def test_bad_input_is_an_error_code():
    from clairs_to_amd._lib import CtoError
    from clairs_to_amd.aspcf import aspcf_windows, exact_pcf, running_median
    rng = np.random.default_rng(1)
    y1, y2 = fresh_tracks(rng, 1001)
    ok = dict(kmin=6, gamma=50, where="host")
    aspcf_windows(y1, y2, [0], [1000], [0.01], [0.01], **ok)
    with pytest.raises(CtoError, match="more than 1000"):
        aspcf_windows(y1, y2, [0], [1001], [0.01], [0.01], **ok)
    with pytest.raises(CtoError, match="divisors"):
        aspcf_windows(y1, y2, [0], [100], [0.0], [0.01], **ok)
    with pytest.raises(CtoError, match="divisors"):
        aspcf_windows(y1, y2, [0], [100], [0.01], [np.nan], **ok)
    with pytest.raises(CtoError, match="not within"):
        aspcf_windows(y1, y2, [900], [1100], [0.01], [0.01], **ok)
    with pytest.raises(CtoError, match="kmin"):
        aspcf_windows(y1, y2, [0], [100], [0.01], [0.01], 0, 50, "host")
    bad = y1.copy()
    bad[500] = np.nan
    with pytest.raises(CtoError, match="NaN"):
        aspcf_windows(bad, y2, [0], [100], [0.01], [0.01], **ok)
    with pytest.raises(CtoError, match="NaN"):
        aspcf_windows(y1, bad, [0], [100], [0.01], [0.01], **ok)
    with pytest.raises(CtoError, match="NaN"):
        running_median(bad, 25)
    with pytest.raises(CtoError, match="NaN"):
        exact_pcf(bad, 6, 50)
