"""predict_germline_genotypes with the window distances on the device (csrc/germline.hip) against the reference
(tests/golden/verdict_gg.json.gz): every scenario's argv through the dispatch of `python -m clairs_to_amd predict_germline_genotypes`, byte
for byte; and, on arrays freshly seeded every run, the kernel's distances against the host path of the same call, bit for bit, over
the run lengths and segment lengths at which the kernel takes another path."""
import os
import random

import numpy as np
import pytest

import verdictsim
from conftest import load_json_gz
from test_verdict_gg import fresh_runs, same_bits, write_files

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load_json_gz("verdict_gg.json.gz")


def test_every_scenario_byte_for_byte_on_the_device(golden, tmp_path, monkeypatch):
    from clairs_to_amd.__main__ import dispatch
    from clairs_to_amd.predict_germline_genotypes import predict_germline_genotypes
    files = verdictsim.baf_files(golden["gg"]["spec"])
    assert verdictsim.digest(files) == golden["gg"]["inputs_sha256"]
    write_files(str(tmp_path), files)
    monkeypatch.chdir(tmp_path)
    assert len(golden["gg"]["runs"]) == 6
    for run in golden["gg"]["runs"]:
        dispatch("predict_germline_genotypes", list(run["argv"]) + ["--where", "device"])
        for fn, text in run["outputs"].items():
            assert open(fn).read() == text, run["name"]
            os.remove(fn)
    st = {}                                                    # the defaults again, for the call's own account of where it ran
    predict_germline_genotypes("logr.txt", "baf.txt", None, "again.txt", sample_name="TUM", where="device", stats=st)
    assert open("again.txt").read() == golden["gg"]["runs"][0]["outputs"]["out_GG.txt"]
    assert st["host_path"] == 0 and st["kernel_ms"] > 0 and st["n_runs"] == len(golden["gg"]["spec"]["runs"])
    assert st["n_probes"] == golden["gg"]["runs"][0]["cut"]["undecided"]


def shapes(rng, tile):
    """the run lengths of the issue; a run that ends on a tile seam followed, one probe later, by one that starts one past it; two and a
    bit tiles; lengths drawn fresh"""
    return [0, 1, 5, 6, 7, 12, 101, 102, 300, tile, 1, tile + 1, 2 * tile, 2 * tile + 3, int(rng.integers(6, 3 * tile)), 0, 3]


@pytest.mark.parametrize("segment_length", [2, 3, 7, 100, "cap"])
def test_device_distances_are_the_host_s_bits(segment_length):
    from clairs_to_amd.predict_germline_genotypes import GG_MAX_SEGMENT, GG_TILE, window_dist
    if segment_length == "cap":
        segment_length = GG_MAX_SEGMENT
    seed = random.SystemRandom().randrange(1 << 30)
    print("seed", seed)
    rng = np.random.default_rng(seed)
    ms = shapes(rng, GG_TILE)
    c, off = fresh_runs(rng, ms)
    sd, sh = {}, {}
    dev = window_dist(c, off, segment_length, "device", sd)
    host = window_dist(c, off, segment_length, "host", sh)
    assert sd["host_path"] == 0 and sh["host_path"] == 1 and sd["n_probes"] == len(c) and sd["n_runs"] == len(ms)
    assert same_bits(dev, host), (seed, np.nonzero(dev.view(np.uint64) != host.view(np.uint64))[0][:5])
    assert np.isinf(dev).any() == (segment_length >= 5) and (dev[off[2]:off[3]] == 1.0).all()


def test_a_segment_length_above_the_cap_takes_the_host_path():
    from clairs_to_amd.predict_germline_genotypes import GG_MAX_SEGMENT, window_dist
    rng = np.random.default_rng(3)
    c, off = fresh_runs(rng, [700, 40, GG_MAX_SEGMENT + 2])
    st = {}
    got = window_dist(c, off, GG_MAX_SEGMENT + 1, "device", st)
    assert st["host_path"] == 1 and st["kernel_ms"] == 0.0
    assert same_bits(got, window_dist(c, off, GG_MAX_SEGMENT + 1, "host"))
    at_cap = {}
    window_dist(c, off, GG_MAX_SEGMENT, "device", at_cap)
    assert at_cap["host_path"] == 0


def test_bad_input_is_an_error_code_not_a_wrong_answer():
    from clairs_to_amd._lib import CtoError
    from clairs_to_amd.predict_germline_genotypes import window_dist
    c = np.full(300, 0.4)
    c[123] = np.nan
    with pytest.raises(CtoError, match="NaN"):
        window_dist(c, [0, 300], 100, "device")
    with pytest.raises(CtoError, match="ascend"):
        window_dist(np.full(300, 0.4), [0, 200, 100, 300], 100, "device")
    with pytest.raises(CtoError, match="below 2"):
        window_dist(np.full(300, 0.4), [0, 300], 1, "device")
