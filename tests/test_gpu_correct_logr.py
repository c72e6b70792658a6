"""correct_logr with the fit on the device (csrc/correctlogr.hip): every scenario of tests/golden/correct_logr.json.gz through the dispatch
of `python -m clairs_to_amd correct_logr`, the same bytes as the host path's file and the reference's decisions and accuracy condition;
and, on tables freshly seeded every run, the kernels against the host path of the same call, bit for bit - the chosen columns, the
correlations with their NaNs, every residual - over the row counts on both sides of a block of the summation tree and the column counts
at which the table kernels' steps change shape; rows exactly at a chosen column's ends and middle knot; what is refused."""
import ctypes as C
import os
import random

import numpy as np
import pytest

from conftest import load_json_gz
from test_correct_logr import OUTPUT, SCENARIOS, check_against_reference, fresh_tables, scenario, write_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load_json_gz("correct_logr.json.gz")


def raw_call(logr, gc, rt, where):
    """cto_correct_logr as it returns: (code, message, corr_gc, corr_rt, residual, stats) - the arrays as far as a failing call filled them"""
    from clairs_to_amd._lib import CorrectLogrStats, lib
    logr, gc, rt = [np.ascontiguousarray(v, dtype=np.float64) for v in (logr, gc, rt)]
    corr_gc, corr_rt, residual, st = np.zeros(gc.shape[1]), np.zeros(rt.shape[1]), np.zeros(len(logr)), CorrectLogrStats()
    rc = lib.cto_correct_logr(logr.ctypes.data, len(logr), gc.ctypes.data, gc.shape[1], rt.ctypes.data, rt.shape[1], 0 if where == "device" else 1,
                              corr_gc.ctypes.data, corr_rt.ctypes.data, residual.ctypes.data, C.byref(st))
    return rc, lib.cto_last_error().decode() if rc else "", corr_gc, corr_rt, residual, {name: getattr(st, name) for name, _ in CorrectLogrStats._fields_}


def both_paths(logr, gc, rt, note):
    dev, host = raw_call(logr, gc, rt, "device"), raw_call(logr, gc, rt, "host")
    assert dev[:2] == host[:2], note
    for k in (2, 3, 4):
        assert (dev[k].view(np.uint64) == host[k].view(np.uint64)).all(), (note, k, np.argwhere(dev[k].view(np.uint64) != host[k].view(np.uint64))[:5])
    sd, sh = dev[5], host[5]
    assert sd["host_path"] == 0 and sh["host_path"] == 1 and sh["kernel_ms"] == 0.0
    assert {k: v for k, v in sd.items() if k not in ("host_path", "kernel_ms")} == {k: v for k, v in sh.items() if k not in ("host_path", "kernel_ms")}, note
    return dev


@pytest.mark.parametrize("name", SCENARIOS)
def test_every_scenario_on_the_device(golden, name, tmp_path, monkeypatch):
    from clairs_to_amd.__main__ import dispatch
    from clairs_to_amd.correct_logr import correct_logr
    sc = scenario(golden, name)
    write_inputs(str(tmp_path), sc)
    monkeypatch.chdir(tmp_path)
    if sc["output"] is None:
        with pytest.raises(SystemExit) as e:
            dispatch("correct_logr", list(sc["argv"]) + ["--where", "device"])
        assert repr(tuple(sc["missing"])) in str(e.value.code) and not os.path.exists(OUTPUT)
        return
    dispatch("correct_logr", list(sc["argv"]) + ["--where", "device"])
    text = open(OUTPUT).read()
    sd, sh = {}, {}
    correct_logr("logr.txt", "gc.txt", "rt.txt", "device.txt", "TUM", "device", sd)
    correct_logr("logr.txt", "gc.txt", "rt.txt", "host.txt", "TUM", "host", sh)
    assert open("device.txt").read() == text == open("host.txt").read()
    assert sd["host_path"] == 0 and sd["kernel_ms"] > 0 and sh["host_path"] == 1
    check_against_reference(sc, text, sd)


@pytest.mark.parametrize("columns", [(8, 1), (12, 2), (13, 16), (25, 12)])
@pytest.mark.parametrize("rows", ["2", "40", "B-1", "B", "B+1", "2B+1", "fresh"])
def test_the_device_returns_the_host_path_s_bits(rows, columns):
    from clairs_to_amd.correct_logr import BLOCK_ROWS
    seed = random.SystemRandom().randrange(1 << 30)
    rng = np.random.default_rng(seed)
    B = BLOCK_ROWS
    n = {"2": 2, "40": 40, "B-1": B - 1, "B": B, "B+1": B + 1, "2B+1": 2 * B + 1, "fresh": int(rng.integers(3000, 20001))}[rows]
    print("seed", seed, "rows", n)
    g, t = columns
    rc, msg, corr_gc, corr_rt, residual, st = both_paths(*fresh_tables(rng, n, g, t), (seed, n, columns))
    if n == 2:                                                   # twelve columns on two rows: the factor's first pivot that is not positive
        assert rc < 0 and "pivot" in msg and not np.isnan(corr_gc).any()
        return
    assert rc == 0 and st["kernel_ms"] > 0 and st["n_rows"] == n and (st["n_gc"], st["n_rt"]) == columns, msg
    assert 0 <= st["col_insert"] < min(6, g) and 7 <= st["col_amplic"] < min(12, g) and 0 <= st["col_replic"] < t
    assert np.isfinite(residual).all() and residual.std() > 0 and abs(residual.sum()) < 1e-9 * n


def test_rows_at_the_ends_and_the_middle_knot_and_a_constant_column():
    """the choice is forced: GC columns 3 and 9 repeat column 0 (entries 2 and 8 of the row are 1), RT column 2 is constant (entry 1 is
    NaN, and np.argmax takes it); GC column 7 is constant too, its entry 6 outside both windows"""
    seed = random.SystemRandom().randrange(1 << 30)
    print("seed", seed)
    rng = np.random.default_rng(seed)
    n = 1500
    logr, gc, rt = fresh_tables(rng, n, 14, 3)
    gc[:, 3] = gc[:, 9] = gc[:, 0]
    gc[:, 7] = 0.25
    rt[:, 2] = -2.0
    for col in (gc[:, 2], gc[:, 8], rt[:, 1]):
        lo, hi = col.min(), col.max()
        mid = (hi - lo) / 2.0 + lo
        at = rng.choice(n, size=11, replace=False)
        col[at[:3]], col[at[3:6]], col[at[6:9]], col[at[9]], col[at[10]] = lo, hi, mid, np.nextafter(mid, lo), np.nextafter(mid, hi)
    rc, msg, corr_gc, corr_rt, residual, st = both_paths(logr, gc, rt, seed)
    assert rc == 0, msg
    assert (st["col_insert"], st["col_amplic"], st["col_replic"]) == (2, 8, 1)
    assert np.isnan(corr_gc[6]) and np.isnan(corr_rt[1]) and np.isnan(corr_gc).sum() == 1 and np.isnan(corr_rt).sum() == 1
    assert np.isfinite(residual).all()


def test_bad_input_is_an_error_code_on_the_device_path():
    from clairs_to_amd._lib import CtoError
    from clairs_to_amd.correct_logr import fit
    rng = np.random.default_rng(17)
    logr, gc, rt = fresh_tables(rng, 600, 9, 2)
    with pytest.raises(CtoError, match="1 rows"):
        fit(logr[:1], gc[:1], rt[:1], "device")
    with pytest.raises(CtoError, match="7 GC columns"):
        fit(logr, gc[:, :7], rt, "device")
    bad = logr.copy()
    bad[431] = np.inf
    with pytest.raises(CtoError, match="not finite"):
        fit(bad, gc, rt, "device")
    flat = gc.copy()
    flat[:, 0] = 0.5
    with pytest.raises(CtoError, match="column 0 of the GC table, chosen for the fit, is constant"):
        fit(logr, flat, rt, "device")
    for tables in ((bad, gc, rt), (logr, flat, rt)):
        assert both_paths(*tables, "refused")[0] < 0
    st = {}
    assert fit(logr, gc, rt, "device", st)[2].shape == (600,) and st["host_path"] == 0      # and the call after a refusal is sound
