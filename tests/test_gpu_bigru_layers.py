"""The BiGRU kernels (csrc/gru_kernel.h, csrc/gru_split_kernel.h, launched from csrc/gru.hip) layer by layer, and at batches that leave
the first launch range.  Every other test sees them through the finished network - after fc1 (K = 12 672), three SELUs and the heads,
at 1e-4 - and at batches of at most one round of workgroups.  Here cto_debug_bigru_layers hands out what a forward left behind:

  h1    layer 1's output [B][33][256], against torch.nn.GRU in float64 on the CPU (tests/bigruutil.py);
  slab  the fc1 partial sums [2][B][128] of the fused layer-2 kernel, against float64 - the layer-2 reference is fed the DEVICE's
        layer-1 output, so layer 2 is judged by itself;
  h2    layer 2's state, which the kernel never writes: six fc1 sets whose weight is one-hot make the slab show 768 of its elements per
        direction (every hidden unit, every step, both ends of each direction) - the sum's other terms are exact zeros.

Bars (bigruutil.BARS).  A kernel's worst distance from float64 is counted in units of the float32 twin's distance from float64 - the
same torch modules in float32 on the same inputs and weights, recomputed in each test.  What sets a kernel apart from the twin is the
1-ulp v_exp / v_rcp forms and the MFMA summation order, a small constant factor; the bar is twice the worst multiple measured on
MI355X (256 CUs), rounded up.  Measured, worst over the tests of this file (printed with -s as MULT lines), and the bar in brackets:

    kernel   weights   h1           h2           slab
    fp32     x1        1.54  (4)    2.18  (5)    7.75  (16)
    fp32     x3        1.50  (3)    1.82  (4)    4.80  (10)
    f16      x1        5.95  (12)   0.80  (2)    3.72  (8)
    bf16     x1        93.7  (188)  12.6  (26)   11.3  (23)

In absolute terms the fp32 kernels sit 2e-7 .. 3e-7 from float64 on both layers where the activations are O(1) (golden windows, x1),
1e-5 on layer 1 where unrescaled 8 000-deep windows and x3 weights drive it, and 2e-6 .. 4e-6 on the dense slab.  The slab is the one
quantity on which the fp32 kernel is several times the twin: the kernel adds the 6 336 products of a direction into ONE fp32
accumulator, in order, where the twin's BLAS sums in blocks - a chain of 6 336 rounded fused multiply-adds restated on the CPU sits
3.5 .. 4.7 x the twin from float64 on such inputs (2.7e-6), which is where the device is.  No fp32 figure exceeds the 16 x beyond
which the distance would be a finding and not a bar (bigruutil.FP32_CEILING).  f16 / bf16 halves carry 22 / 16-17 significant bits
into layer 1, whose inputs here reach 12 000 counts; the split kernels are judged at x1 only.

Exact, whatever the arithmetic: a site's h1, slabs and logits do not depend on the batch around it (whole batch against pieces that
run as 16-site tiles); layer 1 on the int16 tensor equals layer 1 on the fp32 hand-over; what two selector sets show of the same
element is the same bits.

Shapes.  Small batches 1 .. 97 over the fixture windows (whole, partial and single-row 16-site tiles).  Geometry, with rnd = 16 x CUs
the sites of one round: 3 rnd / 4 (the last batch of 16-site tiles), + 1 (the first of 32-site tiles, one live row in the last), + 29
(a ragged 32-site tile whose second half is partial), rnd + 17 (a second launch range, begin = rnd, of 16-site tiles),
rnd + 3 rnd / 4 + 29 (a second range of ragged 32-site tiles), 2 rnd + 1 (two whole rounds in the first range).  Each test asserts
with the restated launch rule that its batch runs as the ranges it is meant for."""
import numpy as np
import pytest

import bigruutil as U
from conftest import load_models_npz
from weights_recipe import make_weights

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cus(dev):
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


class Net:
    """one BiGRU handle: forwards on poisoned LDS, then the layers through the debug accessor"""

    def __init__(self, w, cls="BiGRU_NACGT", split=None):
        from clairs_to_amd._lib import lib
        from clairs_to_amd.nn_shims import from_state_dict
        self.m = from_state_dict(cls, w)
        self.m.split_operands = split or "f32"
        self.h = self.m._handle()
        self.K = int(lib.cto_model_n_out(self.h))

    def run(self, xd, raw=None):
        """(logits [K][B][2], h1 [B][33][256], slab [2][B][128]) on the device; raw = (site_info, which, cov): xd is the int16 tensor"""
        import torch
        from clairs_to_amd._lib import lib, check, current_stream_ptr
        B, dev = xd.shape[0], xd.device
        logits, h1, slab = torch.empty((self.K, B, 2), device=dev), torch.empty((B, U.T, 2 * U.H1), device=dev), torch.empty((2, B, U.NF), device=dev)
        s = current_stream_ptr()
        check(lib.cto_debug_poison_lds(s))
        if raw is None:
            assert xd.dtype == torch.float32 and xd.is_contiguous()
            check(lib.cto_model_forward(self.h, xd.data_ptr(), B, logits.data_ptr(), s))
        else:
            assert xd.dtype == torch.int16 and xd.is_contiguous() and raw[0].dtype == torch.int32
            check(lib.cto_model_forward_raw(self.h, xd.data_ptr(), raw[0].data_ptr(), raw[1], raw[2], B, logits.data_ptr(), s))
        check(lib.cto_debug_bigru_layers(self.h, B, h1.data_ptr(), slab.data_ptr(), s))
        torch.cuda.synchronize()
        return logits, h1, slab


_NETS = {}


def net(scale=1.0, fc="dense", split=None, cls="BiGRU_NACGT"):
    """fc: "dense" (the recipe's fc1) or a selector set 0 .. 5 (one-hot, NOT scaled with the other matrices)"""
    key = (scale, fc, split, cls)
    if key not in _NETS:
        w = U.recipe_weights(cls, scale)
        if fc != "dense":
            w = dict(w, **{"fc1.weight": U.selector_fc1(fc)})
        _NETS[key] = (Net(w, cls, split), w)
    return _NETS[key]


@pytest.fixture(scope="module", autouse=True)
def _drop_nets():
    yield
    _NETS.clear()


def judge(tag, kernel, quantity, got, want64, twin32, bad):
    """got's worst distance from float64 in units of the float32 twin's; prints the multiple, notes a miss of the bar in `bad`"""
    got, twin32 = np.asarray(got, dtype=np.float64), np.asarray(twin32, dtype=np.float64)
    assert got.shape == want64.shape == twin32.shape and np.isfinite(got).all(), (tag, quantity)
    d, unit = float(np.abs(got - want64).max()), float(np.abs(twin32 - want64).max())
    assert unit > 0, (tag, quantity)
    print("\nMULT %-5s x%d %-4s %-40s |d| %.3e  twin %.3e  multiple %.2f" % (kernel[0], kernel[1], quantity, tag, d, unit, d / unit), end="")
    if not d <= U.BARS[kernel][quantity] * unit:
        bad.append((tag, kernel, quantity, d, unit, d / unit))
    if kernel[0] == "f32":
        assert U.BARS[kernel][quantity] <= U.FP32_CEILING


def layer_refs(w, x, h1_dev):
    """float64 reference and float32 twin of both layers for the sites x; layer 2 is fed the device's own layer-1 output"""
    import torch
    r = {"h1_64": U.torch_layer(w, "lstm", x, torch.float64), "h1_32": U.torch_layer(w, "lstm", x, torch.float32)}
    r["h2_64"], r["h2_32"] = U.torch_layer(w, "lstm_2", h1_dev, torch.float64), U.torch_layer(w, "lstm_2", h1_dev, torch.float32)
    return r


def judge_slab(tag, kernel, fc, w, r, slab, bad, rows=slice(None)):
    """a slab [2][n][128] of the sites `rows` of r: the dense fc1 sums, or the elements of layer 2's state a selector set shows"""
    if fc == "dense":
        judge(tag, kernel, "slab", slab, U.fc1_partials(r["h2_64"][rows], w["fc1.weight"]), U.fc1_partials(r["h2_32"][rows], w["fc1.weight"]), bad)
    else:
        judge(tag + " sel %d" % fc, kernel, "h2", slab, U.selector_pick(r["h2_64"][rows], fc), U.selector_pick(r["h2_32"][rows], fc), bad)


def assert_selector_identity(slabs):
    """slabs: selector set -> [2][B][128] device tensor; set 5 shows again, at other outputs, what sets 0-4 show: the same bits"""
    import torch
    for n in range(U.NF):
        if n % 5 in slabs and 5 in slabs:
            assert torch.equal(slabs[5][:, :, n], slabs[n % 5][:, :, 127 - n]), n


# ---------------------------------------------------------------- small batches
SMALL = (1, 15, 16, 17, 31, 33, 97)


@pytest.mark.parametrize("scale", [1.0, 3.0])
def test_small_batches_layer_by_layer(dev, cus, scale):
    """B = 1 .. 97 over the fixture windows, recipe weights x1 and x3 (x3 saturates the gates: __expf overflows to inf, which rcp has to
    turn into 0 or 1), the dense fc1 and the six selector sets; each batch judged in the twin's unit on ITS windows (up to B = 33
    these are golden windows with O(1) activations, B = 97 adds the 8 000-deep, all-zero, one-hot and 1/1024 ones)"""
    import torch
    x = U.fixture_windows()
    assert len(x) == 97
    xd = torch.from_numpy(x).to(dev)
    dense, w = net(scale)
    _, h1_all, slab_all = dense.run(xd)
    r = layer_refs(w, x, h1_all.cpu().numpy())
    bad = []
    for B in SMALL:
        tag = "x%g B=%d" % (scale, B)
        logits, h1, slab = dense.run(xd[:B].contiguous())
        assert torch.isfinite(logits).all()
        assert torch.equal(h1, h1_all[:B]) and torch.equal(slab, slab_all[:, :B]), tag         # 16-site tiles either way: the same bits
        judge(tag, ("f32", int(scale)), "h1", h1.cpu().numpy(), r["h1_64"][:B], r["h1_32"][:B], bad)
        judge_slab(tag, ("f32", int(scale)), "dense", w, r, slab.cpu().numpy(), bad, slice(0, B))
        sel = {}
        for s in range(U.N_SELECTORS):
            sn, sw = net(scale, s)
            _, h1_s, sel[s] = sn.run(xd[:B].contiguous())
            assert torch.equal(h1_s, h1), (tag, s)
            judge_slab(tag, ("f32", int(scale)), s, sw, r, sel[s].cpu().numpy(), bad, slice(0, B))
        assert_selector_identity(sel)
    assert not bad, bad


def test_indel_class_runs_the_same_layers(dev):
    """BiGRU_NACGT_Indel: the same two layers under a six-way head, with its own recipe weights"""
    import torch
    x = U.fixture_windows()
    n, w = net(cls="BiGRU_NACGT_Indel")
    assert n.K == 6
    logits, h1, slab = n.run(torch.from_numpy(x).to(dev))
    assert torch.isfinite(logits).all()
    r = layer_refs(w, x, h1.cpu().numpy())
    bad = []
    judge("indel B=97", ("f32", 1), "h1", h1.cpu().numpy(), r["h1_64"], r["h1_32"], bad)
    judge_slab("indel B=97", ("f32", 1), "dense", w, r, slab.cpu().numpy(), bad)
    assert not bad, bad


def test_debug_accessor_arguments(dev):
    import torch
    from clairs_to_amd._lib import lib, current_stream_ptr
    from clairs_to_amd.nn_shims import from_state_dict
    n, _ = net()
    x = torch.from_numpy(U.fixture_windows()[:5]).to(dev)
    _, h1, slab = n.run(x)
    s = current_stream_ptr()
    only_h1, only_slab = torch.zeros_like(h1), torch.zeros_like(slab)
    assert lib.cto_debug_bigru_layers(n.h, 5, only_h1.data_ptr(), None, s) == 0 and lib.cto_debug_bigru_layers(n.h, 5, None, only_slab.data_ptr(), s) == 0
    torch.cuda.synchronize()
    assert torch.equal(only_h1, h1) and torch.equal(only_slab, slab)
    assert lib.cto_debug_bigru_layers(n.h, 1 << 30, only_h1.data_ptr(), None, s) == -1      # more sites than the workspace ever held: refused before any copy
    g = load_models_npz("CvT")
    cvt = from_state_dict("CvT", make_weights(g["manifest"], seed=g["n_out"]))
    assert lib.cto_debug_bigru_layers(cvt._handle(), 1, only_h1.data_ptr(), None, s) == -1
    assert lib.cto_debug_bigru_layers(None, 1, only_h1.data_ptr(), None, s) == -1


# ---------------------------------------------------------------- launch geometry
def pieces(cus, B):
    """cuts of [0, B) into batches of at most 3/4 of a round, all of which run as 16-site tiles"""
    q = 3 * 16 * cus // 4
    cuts = list(range(0, B, q)) + [B]
    for a, b in zip(cuts[:-1], cuts[1:]):
        assert U.tile_ranges(cus, b - a) == [(0, b - a, 16)]
    return list(zip(cuts[:-1], cuts[1:]))


def whole_against_pieces(n, xd, cus, tag, raw=None):
    """one forward of the whole batch; every piece on its own must give the same bits for its sites"""
    import torch
    B = xd.shape[0]
    logits, h1, slab = n.run(xd, raw)
    assert torch.isfinite(logits).all() and torch.isfinite(h1).all() and torch.isfinite(slab).all(), tag
    for a, b in pieces(cus, B):
        lp, hp, sp = n.run(xd[a:b].contiguous(), None if raw is None else (raw[0][a:b].contiguous(), raw[1], raw[2]))
        assert torch.equal(hp, h1[a:b]), (tag, "h1", a, b)
        assert torch.equal(sp, slab[:, a:b]), (tag, "slab", a, b)
        assert torch.equal(lp, logits[:, a:b]), (tag, "logits", a, b)
    return logits, h1, slab


def geometry(cus, name):
    B, want = U.geometry_shapes(cus)[name]
    assert U.tile_ranges(cus, B) == want, (name, cus, B, U.tile_ranges(cus, B))
    if name in ("second16", "second32", "two_rounds"):
        assert len(want) == 2 and want[1][0] > 0
    return B


def judge_sample(tag, kernel, nets, x, rows, outs, bad):
    """outs: fc -> (h1, slab) device tensors of the whole batch; only the rows of the sample go to the host"""
    import torch
    idx = torch.from_numpy(rows).to(outs["dense"][0].device)
    h1_s = outs["dense"][0][idx].cpu().numpy()
    r = layer_refs(nets["dense"][1], x[rows], h1_s)
    judge(tag, kernel, "h1", h1_s, r["h1_64"], r["h1_32"], bad)
    for fc, (_, slab) in outs.items():
        judge_slab(tag, kernel, fc, nets[fc][1], r, slab[:, idx].cpu().numpy(), bad)


@pytest.mark.parametrize("name", ["last16", "first32", "ragged32", "second16", "second32", "two_rounds"])
def test_launch_geometry(dev, cus, name):
    """(i) whole batch against pieces, bit for bit, on the device; (ii) a sample of at most 128 sites against float64: rows 0, 15, 16,
    31, 32, every row of the last tile of each range, begin - 1, begin, B - 1, random rows; (iii) finite, batch-invariant logits.
    Dense fc1 and selector sets 0 and 5 (5 repeats 0-4 at other outputs)."""
    import torch
    B = geometry(cus, name)
    x = U.resampled_windows(B)
    xd = torch.from_numpy(x).to(dev)
    rows = U.sample_rows(cus, B)
    assert len(rows) <= 128
    nets = {fc: net(1.0, fc) for fc in ("dense", 0, 5)}
    outs = {}
    for fc, (n, _) in nets.items():
        _, h1, slab = whole_against_pieces(n, xd, cus, "%s fc %s" % (name, fc))
        outs[fc] = (h1, slab)
        assert torch.equal(h1, outs["dense"][0])
    assert_selector_identity({0: outs[0][1], 5: outs[5][1]})
    bad = []
    judge_sample("%s B=%d" % (name, B), ("f32", 1), nets, x, rows, outs, bad)
    assert not bad, bad


@pytest.mark.parametrize("cov", [50, 0])
@pytest.mark.parametrize("name", ["ragged32", "second16"])
def test_int16_loader_beyond_one_round(dev, cus, name, cov):
    """layer 1 on the int16 tensor (XRAW: scale rows per tile, indexed by site0 + row) against the fp32 hand-over
    float(double(v) * cov / depth): h1, slabs and logits bit for bit; depths on both sides of min_rescale_cov = 50, the other pass's
    depth column filled with values that would rescale differently"""
    import torch
    B = geometry(cus, name)
    rng = np.random.default_rng(B + cov)
    raw = rng.integers(-60, 121, size=(B, U.T, U.C)).astype(np.int16)
    raw[rng.integers(0, B, size=64), rng.integers(0, U.T, size=64), rng.integers(0, U.C, size=64)] = rng.choice([-32767, 32767, 8000], size=64)
    which = 1
    info = rng.integers(0, 1 << 20, size=(B, 12)).astype(np.int32)
    depth = rng.integers(1, 200, size=B)
    depth[[0, 15, 16, 31, 32, B - 33, B - 17, B - 2, B - 1]] = [49, 50, 51, 50, 8000, 51, 50, 49, 51]
    info[:, 1 + which] = depth
    info[:, 2 - which] = rng.integers(51, 400, size=B)
    assert (depth > 50).mean() > 0.5 and (depth <= 50).mean() > 0.1
    sc = np.where((cov > 0) & (depth > cov), np.float64(cov) / depth.astype(np.float64), 1.0)
    x = (raw.astype(np.float64) * sc[:, None, None]).astype(np.float32)
    n, _ = net()
    rawd, infod, xd = torch.from_numpy(raw).to(dev), torch.from_numpy(info).to(dev), torch.from_numpy(x).to(dev)
    want = n.run(xd)
    got = whole_against_pieces(n, rawd, cus, "%s raw cov %d" % (name, cov), raw=(infod, which, cov))
    for k, a, b in zip(("logits", "h1", "slab"), got, want):
        assert torch.equal(a, b), (name, cov, k)


@pytest.mark.parametrize("kind", ["f16", "bf16"])
@pytest.mark.parametrize("name", ["ragged32", "second16"])
def test_split_operand_kernels_beyond_one_round(dev, cus, name, kind):
    """both layers on split 16-bit operands: batch invariance bit for bit, finite values, the sample against float64 under the bars
    of that arithmetic (dense fc1 and selector set 0)"""
    import torch
    B = geometry(cus, name)
    x = U.resampled_windows(B)
    xd = torch.from_numpy(x).to(dev)
    rows = U.sample_rows(cus, B)
    nets = {fc: net(1.0, fc, split=kind) for fc in ("dense", 0)}
    outs = {}
    for fc, (n, _) in nets.items():
        _, h1, slab = whole_against_pieces(n, xd, cus, "%s %s fc %s" % (name, kind, fc))
        outs[fc] = (h1, slab)
        assert torch.equal(h1, outs["dense"][0])
    bad = []
    judge_sample("%s B=%d" % (name, B), (kind, 1), nets, x, rows, outs, bad)
    assert not bad, bad
