"""The CvT kernels at widths, head counts and depths beyond the two configurations every other test runs (cvtconfigutil.py lists
the seven and what each reaches): the generic GEMM / LayerNorm / depth-wise / attention kernels at widths without a fused
instantiation, the fused block kernel at 2, 5, 7 and 8 heads and at group shapes 4, 4 + 1 and 1, networks that mix both - against
the fp64 run of the REFERENCE's own modules (tests/golden/models_CvT_configs.npz), bar 1e-4 on logits and on the two-way softmax.

Worst |logit - reference fp64| over B = 1, 19, 37 measured on an MI355X, fused where a kernel exists / CTO_CVT_UNFUSED=1 (the fp32
reference itself: 5.1e-6 .. 1.0e-5; test_cvt_configs.py shows that a dropped head moves a logit by 0.25 at the least):
    A  1.3e-5 / 7.9e-6
    B  3.4e-5 / 1.0e-5
    C  1.0e-5 (no stage has a fused kernel: one path)
    D  5.7e-6 (one path)
    E  5.8e-6 (one path)
    F  2.3e-5 / 9.2e-6
    G  3.6e-6 (one path)
The two-way softmax is off by 6.0e-6 at the most (B, fused).  The fused block kernel sits two to three times further from the fp64 run
than the generic kernels on the same weights: a third of the bar at B, whose stage 3 is five fused blocks deep.
"""
import ctypes as C

import numpy as np
import pytest

from cvtconfigutil import BAR, NAMES, load_cvt_configs, stage_kw, weights_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _module(name):
    """the shim class with the stage keywords, then the recipe weights loaded into its state dict (as
    test_cvt_constructor_default_config_matches_oracle builds its model)"""
    import torch
    from clairs_to_amd import nn_shims
    c = load_cvt_configs()[0][name]
    m = (nn_shims.CvT if c["n_out"] == 4 else nn_shims.CvT_Indel)(model_type="acgt", **stage_kw(c["cfg"])).eval()
    sd = m.state_dict()
    for k, v in weights_of(name).items():
        assert tuple(sd[k].shape) == v.shape, k
        sd[k] = torch.from_numpy(v)
    m.load_state_dict(sd)
    return m, c


def _softmax64(lg):
    lg = np.asarray(lg, dtype=np.float64)
    e = np.exp(lg - lg.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


@pytest.mark.parametrize("unfused", ["0", "1"])
@pytest.mark.parametrize("name", NAMES)
def test_cvt_configs_match_the_reference_modules(dev, monkeypatch, name, unfused):
    """B = 1, 19, 37: smaller than or ragged against the 8- and 16-site tiles of the fused kernel and the 64-row GEMM tile; every
    forward starts on LDS full of NaN patterns.  Under CTO_CVT_UNFUSED=1 A, B and F take the generic kernels at stage-1 head
    counts 2 and 7."""
    import torch
    from clairs_to_amd._lib import lib, check, current_stream_ptr
    monkeypatch.setenv("CTO_CVT_UNFUSED", unfused)
    m, c = _module(name)
    x = torch.from_numpy(load_cvt_configs()[1]).to(dev)
    worst = worst_p = 0.0
    for B in (1, 19, 37):
        check(lib.cto_debug_poison_lds(current_stream_ptr()))
        got = m.logits(x[:B]).cpu().numpy()
        assert got.shape == (c["n_out"], B, 2) and np.isfinite(got).all(), (name, unfused, B)
        want = c["logits64"][:, :B]
        d, dp = np.abs(got - want).max(), np.abs(_softmax64(got) - _softmax64(want)).max()
        print("config %s CTO_CVT_UNFUSED=%s B=%2d: |dlogit| %.3g  |dP| %.3g" % (name, unfused, B, d, dp))
        worst, worst_p = max(worst, d), max(worst_p, dp)
    print("config %s CTO_CVT_UNFUSED=%s worst: |dlogit| %.3g  |dP| %.3g" % (name, unfused, worst, worst_p))
    assert worst < BAR and worst_p < BAR, (name, unfused, worst, worst_p)


@pytest.mark.parametrize("name", ["C", "F", "G"])
def test_cvt_configs_are_batch_invariant(dev, name):
    """a site's logits do not depend on which other sites share its launch: bit-equal across groupings, the property
    test_batch_invariance_across_tile_mixes holds for the on-grid model - here with generic stages (C, G) and with fused and generic
    stages in one network (F)"""
    import torch
    m, _ = _module(name)
    x = torch.from_numpy(load_cvt_configs()[1]).to(dev)
    full = m.logits(x)
    parts = torch.cat([m.logits(x[a:b].contiguous()) for a, b in ((0, 1), (1, 20), (20, 37))], dim=1)
    assert torch.isfinite(full).all() and torch.equal(full, parts)


def test_off_grid_config_through_the_other_entry_points(dev):
    """configuration C (no stage on a fused geometry): the custom op on packed weights in manifest order, the C ABI on a handle built
    by state_dict name, and cto_model_forward_raw on the int16 tensor - whose stage 1 has no in-block embedding, so the tensor is
    expanded inside the call - all give the module's bits"""
    import torch
    from clairs_to_amd._lib import lib, check, model_manifest, current_stream_ptr
    from clairs_to_amd.featurize import featurize
    from clairs_to_amd.pack import DevicePack
    from clairs_to_amd.synth import SynthChunk
    from test_gpu_raw_inputs import _logits
    m, c = _module("C")
    w, K = weights_of("C"), c["n_out"]
    x = torch.from_numpy(load_cvt_configs()[1]).to(dev)
    want = m.logits(x)
    cfg = m._cfg()
    packed = torch.from_numpy(np.concatenate([w[k].reshape(-1) for k, n in model_manifest(0, cfg)])).to(dev)
    cfg_list = list(c["cfg"]["emb_dim"]) + list(c["cfg"]["heads"]) + list(c["cfg"]["depth"]) + [K]
    assert torch.equal(torch.ops.clairsto.cvt_forward(x, packed, cfg_list), want)
    out = torch.empty_like(want)
    check(lib.cto_model_forward(m._handle(), x.data_ptr(), x.shape[0], out.data_ptr(), current_stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    # the int16 tensor of a synthetic chunk, rescale on (most sites deeper than 50) and off
    chunk = SynthChunk(37, seed=31, depth_mean=70.0)
    dp, sp = DevicePack(chunk.arrays(), dev), torch.from_numpy(chunk.site_pos).to(dev)
    for cov in (50, 0):
        feat = featurize(dp, sp, 20, cov, want_raw=True, want_x=True)
        if cov:
            assert float((feat.site_info[:, 1] > cov).float().mean()) > 0.5
        for B in (37, 1, 19):
            got = _logits(m._handle(), True, feat, 0, cov, B, K, dev)
            assert np.isfinite(got).all()
            np.testing.assert_array_equal(got, _logits(m._handle(), False, feat, 0, cov, B, K, dev), err_msg="B %d cov %d" % (B, cov))


def test_create_refuses_what_the_kernels_do_not_cover(dev):
    """emb_dim 0, 6, 130, 132, heads 0, 9 and depth 0, in every stage: CTO_EUNSUPPORTED with a message that names the stage, no
    crash; a valid create straight afterwards works and computes"""
    import torch
    from clairs_to_amd._lib import lib, check, CvtCfg, c_vp, current_stream_ptr
    cfgs, x = load_cvt_configs()
    c = cfgs["D"]
    w = c_vp(lib.cto_weights_new())
    try:
        for k, v in weights_of("D").items():
            a = np.ascontiguousarray(v, dtype=np.float32)
            check(lib.cto_weights_add(w, k.encode(), a.ctypes.data, a.size))

        def make(**bad):
            cfg = CvtCfg()
            cfg.emb_dim[:], cfg.heads[:], cfg.depth[:], cfg.n_out = c["cfg"]["emb_dim"], c["cfg"]["heads"], c["cfg"]["depth"], c["n_out"]
            for field, (si, v) in bad.items():
                getattr(cfg, field)[si] = v
            out = c_vp()
            return lib.cto_cvt_create(w, C.byref(cfg), C.byref(out)), out

        for si in range(3):
            for field, values in (("emb_dim", (0, 6, 130, 132)), ("heads", (0, 9)), ("depth", (0,))):
                for v in values:
                    rc, out = make(**{field: (si, v)})
                    assert rc == -4 and not out.value, (si, field, v, rc)                   # CTO_EUNSUPPORTED
                    assert ("stage %d" % (si + 1)).encode() in lib.cto_last_error()
        rc, out = make()
        assert rc == 0 and out.value, lib.cto_last_error()
        try:
            xd = torch.from_numpy(x[:5]).to(dev)
            got = torch.empty((c["n_out"], 5, 2), device=dev)
            check(lib.cto_model_forward(out, xd.data_ptr(), 5, got.data_ptr(), current_stream_ptr()))
            torch.cuda.synchronize()
            assert np.abs(got.cpu().numpy() - c["logits64"][:, :5]).max() < BAR
        finally:
            lib.cto_model_destroy(out)
    finally:
        lib.cto_weights_free(w)
