"""CvT configurations off the two every other fixture pins (cvtconfigutil.py lists them): the CPU oracle and the packed-weights
manifest against what the REFERENCE's own modules gave at those widths, head counts and depths
(tests/golden/models_CvT_configs.npz), and the proof that the GPU parity bar bites where a head loop could stop short."""
import numpy as np
import pytest

from cvtconfigutil import BAR, NAMES, load_cvt_configs, weights_of


@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_the_reference_modules(oracle_lib, name):
    """oracle.cvt_forward within the model bar of the reference module's fp64 run; the fixture's fp32 run lies ten times inside it"""
    cfgs, x = load_cvt_configs()
    c = cfgs[name]
    assert c["logits64"].shape == (c["n_out"], x.shape[0], 2) and c["logits64"].dtype == np.float64
    ref_own = np.abs(c["logits32"] - c["logits64"]).max()
    got = oracle_lib.cvt_forward(weights_of(name), c["cfg"], x)
    worst = np.abs(got - c["logits64"]).max()
    print("config %s: oracle vs ref64 %.3g, ref32 vs ref64 %.3g, max |logit| %.3g" % (name, worst, ref_own, np.abs(c["logits64"]).max()))
    assert ref_own < BAR / 5
    assert np.isfinite(got).all() and worst < BAR


@pytest.mark.parametrize("name", NAMES)
def test_packed_manifest_is_the_reference_state_dict(name):
    """cto_model_manifest names the tensors of the reference module's state_dict, in its order, with its element counts
    (num_batches_tracked, which is no floating-point tensor, aside)"""
    from clairs_to_amd._lib import model_manifest, CvtCfg
    c = load_cvt_configs()[0][name]
    cfg = CvtCfg()
    cfg.emb_dim[:], cfg.heads[:], cfg.depth[:], cfg.n_out = c["cfg"]["emb_dim"], c["cfg"]["heads"], c["cfg"]["depth"], c["n_out"]
    assert model_manifest(0, cfg) == [(k, int(np.prod(s))) for k, s in c["manifest"]]


@pytest.mark.parametrize("name", NAMES)
def test_last_head_of_every_stage_moves_the_logits(oracle_lib, name):
    """Teeth of the GPU parity test: with the q projection of the LAST head of the last block of a stage zeroed (rows
    64 (heads - 1) .. of to_q.net.2.weight), the oracle's logits move by at least 1e-3, ten times the bar, in every stage of every
    configuration - a head loop that stopped one head early would fail the GPU test by that margin."""
    cfgs, x = load_cvt_configs()
    c = cfgs[name]
    w = weights_of(name)
    base = oracle_lib.cvt_forward(w, c["cfg"], x)
    moved = []
    for si in range(3):
        key = "layer%d.2.layers.%d.0.fn.to_q.net.2.weight" % (si + 1, c["cfg"]["depth"][si] - 1)
        heads = c["cfg"]["heads"][si]
        assert w[key].shape[0] == 64 * heads
        cut = dict(w)
        cut[key] = w[key].copy()
        cut[key][64 * (heads - 1):] = 0
        moved.append(float(np.abs(oracle_lib.cvt_forward(cut, c["cfg"], x) - base).max()))
    print("config %s: logits move by %s when a stage's last head is cut; minimum %.3g" % (name, ["%.3g" % v for v in moved], min(moved)))
    assert min(moved) >= 10 * BAR
