"""tests/bigruutil.py checked against itself, without a device: what tests/test_gpu_bigru_layers.py compares the BiGRU kernels with, and
that the comparison can see the slips such kernels make.

  * the numpy restatement of the recurrence equals torch.nn.GRU in float64 (both layers), the fc1 partial sums plus the bias equal
    torch.nn.functional.linear;
  * the six selector fc1 sets are one-hot, show every hidden unit of both directions, every step, each direction's first and last
    step, and their slabs ARE the elements of the layer-2 state they name;
  * every seeded defect (bigruutil.DEFECTS), in the layer the device test would meet it in, moves something that test looks at -
    layer 1's output, the dense fc1 slab, a selector slab - by more than 100 times the bar the device test holds that value to, on the
    same 97 fixture windows and x1 recipe weights.  Measured here (displacement / bar; the fp32 bars of bigruutil.BARS, 4 x / 5 x /
    16 x the float32 twin's 6.8e-6 / 1.0e-6 / 5.2e-7): layer-1 defects 5.9e3 .. 7.3e4 on its output; layer-2 defects 1.0e4 .. 1.1e5 on
    the dense slab, except the chunk of ONE gate row (drop_chunk_one_row) at 1.6e3, and 7e3 .. 2.5e5 on each of the selector sets - no
    defect needs the selector sets to clear the factor, every observation clears it on its own; the table is printed with -s;
  * the batch shapes of the device test land in the launch classes they are meant for, on 256, 304, 64 and 8 compute units, by the
    restated rule and by csrc/gru_tiles.h itself."""
import os
import subprocess

import numpy as np
import pytest

import bigruutil as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref():
    """the 97 windows through both layers: float64 reference, float32 twin, the twin's distances (the units of the bars)"""
    import torch
    x, w = U.fixture_windows(), U.recipe_weights()
    h1_64, h1_32 = U.torch_layer(w, "lstm", x, torch.float64), U.torch_layer(w, "lstm", x, torch.float32)
    h1_in = h1_32                          # the stand-in for the device's layer-1 output that layer 2 is fed in the device test
    h2_64, h2_32 = U.torch_layer(w, "lstm_2", h1_in, torch.float64), U.torch_layer(w, "lstm_2", h1_in, torch.float32)
    slab_64, slab_32 = U.fc1_partials(h2_64, w["fc1.weight"]), U.fc1_partials(h2_32, w["fc1.weight"])
    noise = {"h1": float(np.abs(h1_32 - h1_64).max()), "h2": float(np.abs(h2_32 - h2_64).max()), "slab": float(np.abs(slab_32 - slab_64).max())}
    return dict(x=x, w=w, h1_64=h1_64, h1_in=h1_in, h2_64=h2_64, slab_64=slab_64, noise=noise)


def test_restatement_equals_torch_in_float64(ref):
    for name, x, want in (("lstm", ref["x"], ref["h1_64"]), ("lstm_2", ref["h1_in"], ref["h2_64"])):
        got = U.np_layer(ref["w"], name, x)
        d = float(np.abs(got - want).max())
        print("restatement vs torch float64, %s: %.2e" % (name, d))
        assert got.shape == want.shape and d < 1e-12, (name, d)


def test_fc1_partials_plus_bias_equal_linear(ref):
    import torch
    w = ref["w"]
    h2 = torch.from_numpy(ref["h2_64"])
    want = torch.nn.functional.linear(h2.reshape(h2.shape[0], -1), torch.from_numpy(w["fc1.weight"]).double(),
                                      torch.from_numpy(w["fc1.bias"]).double()).numpy()
    got = ref["slab_64"].sum(axis=0) + w["fc1.bias"].astype(np.float64)
    d = float(np.abs(got - want).max())
    assert ref["slab_64"].shape == (2, len(ref["x"]), 128) and d < 1e-12, d
    np.testing.assert_array_equal(U.np_partials(ref["h2_64"], w["fc1.weight"]), ref["slab_64"])


def test_selector_sets_are_one_hot_and_cover_the_state(ref):
    seen_j, seen_t = [set(), set()], [set(), set()]
    for s in range(U.N_SELECTORS):
        f = U.selector_fc1(s).reshape(U.NF, U.T, 2, U.H2)
        m = U.selector_map(s)
        assert m.shape == (2, 2, U.NF)
        for d in range(2):
            assert set(np.unique(f)) == {0.0, 1.0} and (f[:, :, d].reshape(U.NF, -1).sum(axis=1) == 1).all()       # one (t, j) per output and direction
            seen_t[d] |= set(m[d][0].tolist())
            seen_j[d] |= set(m[d][1].tolist())
        # the slab of a selector set is the state's element itself: every other term of the sum is an exact zero
        np.testing.assert_array_equal(U.fc1_partials(ref["h2_64"], f.reshape(U.NF, -1)), U.selector_pick(ref["h2_64"], s))
    for d in range(2):
        assert seen_j[d] == set(range(U.H2)) and seen_t[d] == set(range(U.T)), d
    first = U.selector_map(0)
    for d in range(2):       # set 0 shows both ends of the recurrence: t = 0 and t = 32 are a direction's first and last step
        assert {0, U.T - 1} <= set(first[d][0][:64].tolist())
    # set 5 shows again what sets 0-4 show, at other outputs
    last = U.selector_map(U.N_SELECTORS - 1)
    for n in range(U.NF):
        np.testing.assert_array_equal(last[:, :, n], U.selector_map(n % 5)[:, :, 127 - n])


def _observed(ref, h1=None, h2=None, defect=None):
    """what the device test looks at, for a layer-1 output or a layer-2 state: name -> (values, bar)"""
    bars, noise = U.BARS[("f32", 1)], ref["noise"]
    if h1 is not None:
        return {"h1": (h1, bars["h1"] * noise["h1"])}
    out = {"slab": (U.np_partials(h2, ref["w"]["fc1.weight"], defect), bars["slab"] * noise["slab"])}
    for s in range(U.N_SELECTORS):
        out["selector %d" % s] = (U.np_partials(h2, U.selector_fc1(s), defect), bars["h2"] * noise["h2"])
    return out


@pytest.fixture(scope="module")
def clean(ref):
    h1, h2 = U.np_layer(ref["w"], "lstm", ref["x"]), U.np_layer(ref["w"], "lstm_2", ref["h1_in"])
    return {1: _observed(ref, h1=h1), 2: _observed(ref, h2=h2)}


@pytest.mark.parametrize("defect,layer", [(d, l) for l in (1, 2) for d in U.DEFECTS if (d, l) != ("reverse_fc1_shift", 1)])     # layer 1 has no fc1
def test_every_seeded_defect_moves_an_observed_value_by_100_bars(ref, clean, defect, layer):
    if layer == 1:
        got = _observed(ref, h1=U.np_layer(ref["w"], "lstm", ref["x"], defect))
    else:
        got = _observed(ref, h2=U.np_layer(ref["w"], "lstm_2", ref["h1_in"], defect), defect=defect)
    factor = {k: float(np.abs(v - clean[layer][k][0]).max()) / bar for k, (v, bar) in got.items()}
    print("DEFECT %-18s layer %d: displacement / bar  %s" % (defect, layer, "  ".join("%s %.3g" % kv for kv in factor.items())))
    assert all(np.isfinite(list(factor.values())))
    # one observation would do; every one of them clears the factor (layer 2: the dense slab and each selector set)
    assert min(factor.values()) > 100, factor


def test_the_noise_units_are_what_float32_gives(ref):
    """the twin's distances on these inputs: ~1e-6 on the layers (the 8 000-deep windows carry them; 2.5e-7 / 4e-7 on O(1) inputs)"""
    print("float32 twin vs float64 on the 97 windows:", ref["noise"])
    for k, v in ref["noise"].items():
        assert 1e-8 < v < 1e-4, (k, v)


@pytest.fixture(scope="module")
def header_ranges(tmp_path_factory):
    """csrc/gru_tiles.h through its stand-alone driver (tests/host/gru_tiles_check.cpp)"""
    exe = str(tmp_path_factory.mktemp("gru_tiles") / "gru_tiles_check")
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "clairs_to_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "gru_tiles_check.cpp"), "-o", exe])

    def run(cus, B):
        out = subprocess.run([exe, str(cus), str(B)], stdout=subprocess.PIPE, check=True).stdout.decode()
        return [(int(a), int(b), 16 * int(ms)) for a, b, ms in (line.split() for line in out.splitlines())]
    return run


@pytest.mark.parametrize("cus", [256, 304, 64, 8])
def test_shapes_land_in_their_launch_classes(header_ranges, cus):
    rnd = 16 * cus
    shapes = U.geometry_shapes(cus)
    assert len(shapes) == 6 and len({B for B, _ in shapes.values()}) == 6
    for name, (B, want) in shapes.items():
        assert U.tile_ranges(cus, B) == want == header_ranges(cus, B), (cus, name, B)
        rows = U.sample_rows(cus, B)
        assert len(rows) == min(B, 128) == len(set(rows.tolist())) and rows.min() >= 0 and rows.max() == B - 1
        for begin, end, th in want:
            last_tile = range(begin + (end - begin - 1) // th * th, end)
            assert set(last_tile) | {begin, max(begin - 1, 0)} <= set(rows.tolist()), (cus, name)
        assert {0, 15, 16, 31, 32} <= set(rows.tolist())
    # the classes by what they are: tile heights, a second range, ragged tiles
    assert shapes["last16"][1][0][2] == 16 and shapes["first32"][1][0][2] == 32 and shapes["first32"][0] % 32 == 1
    assert shapes["ragged32"][0] % 32 == 29 and 16 < shapes["ragged32"][0] % 32 < 32                 # the second sub-tile is partial
    assert shapes["second16"][1][1] == (rnd, rnd + 17, 16) and shapes["second32"][1][1][0] == rnd and shapes["second32"][1][1][2] == 32
    assert (shapes["second32"][0] - rnd) % 32 == 29 and shapes["two_rounds"][1][0] == (0, 2 * rnd, 32)
    # the small batches of the device test all run as 16-site tiles wherever a round holds more than 128 sites
    if cus >= 64:
        for B in (1, 15, 16, 17, 31, 33, 97):
            assert U.tile_ranges(cus, B) == [(0, B, 16)]
