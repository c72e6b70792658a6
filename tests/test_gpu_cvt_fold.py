"""Folded attention weights in the fused CvT block kernel (csrc/cvt_block.h: FOLD; DESIGN.md 7.1 "Folded attention weights") against
the unfolded kernel (CTO_CVT_FOLD=0) and the fp64 runs of the reference network, on the 37 golden rows of cvtconfigutil.py:

  S  16,64,128 / 1,3,4 / 1,2,3 / 4   the default SNV configuration (tests/golden/models_CvT.npz holds its fp32 reference logits; the
                                     fp64 ones come from cvt_fp64.py, which test_cvt_fp64.py ties to the reference's fp64 runs)
  A  16,64,128 / 2,5,8 / 4,5,1 / 4   stage 1 (C = 16) folded with 2 heads, four blocks in one launch; stage 2 with 5 heads, 4 + 1 blocks
  B  32,64,128 / 7,8,2 / 2,1,5 / 6   stage 1 at C = 32 with 7 heads, stage 2 with 8 heads
  F  16,72,128 / 7,3,4 / 1,2,3 / 6   stage 1 folded with 7 heads; stage 2 at C = 72 has no fused kernel and no folded weights

Stages 1 and 2 are folded, stage 3 (C = 128 > dim_head) never is.  F's stage 1 is folded too, so its logits cannot be the same bits under
both settings; what must be is checked where the setting can be told apart from stage 1: with every stage on the generic kernels
(CTO_CVT_UNFUSED=1) the setting changes no bit, and with the fused kernels F meets the same error bound as the others.

The fold replaces two rounded products (q and k; v and the out-projection) by one product with a matrix that was formed in double
and rounded once: the same order of error, not provably smaller, and 37 rows are few - so the folded path may sit at most twice as
far from fp64 as the worse of the unfolded path and the fp32 reference, and under the project's 1e-4 bar.

max |logit - fp64| over the 37 rows on an MI355X, folded / unfolded / the fp32 reference:
    S  1.16e-05 / 1.43e-05 / 5.94e-06        (stage 2 alone folded: 1.70e-05)
    A  1.53e-05 / 1.28e-05 / 6.35e-06        (1.34e-05)
    B  2.30e-05 / 3.42e-05 / 1.01e-05        (3.57e-05)
    F  1.64e-05 / 2.31e-05 / 9.96e-06
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_models_npz
from cvt_fp64 import cvt_forward_fp64
from cvtconfigutil import BAR, load_cvt_configs, stage_kw, weights_of
from weights_recipe import CVT_CFG, make_weights

pytestmark = pytest.mark.gpu

FOLDED = ("S", "A", "B", "F")
EDGES = (1, 7, 8, 9, 15, 16, 17, 33)         # around the 8- and 16-site tiles, ragged last tiles, more than one workgroup


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _config(name):
    """(cfg with n_out, recipe weights, logits32 [K,37,2], logits64 [K,37,2]) of a configuration on the 37 rows"""
    cfgs, x = load_cvt_configs()
    if name != "S":
        c = cfgs[name]
        return c["cfg"], weights_of(name), c["logits32"], c["logits64"]
    g = load_models_npz("CvT")
    rows = np.load(os.path.join(GOLDEN, "models_CvT_configs.npz"))["rows"]
    cfg, w = dict(CVT_CFG, n_out=g["n_out"]), make_weights(g["manifest"], seed=g["n_out"])
    return cfg, w, g["logits"][:, rows], cvt_forward_fp64(w, cfg, x)


class _Paths:
    """one module per (configuration, CTO_CVT_FOLD) and its logits on the 37 rows, computed once; the setting is read when a handle is
    created and is part of the shim's handle key, so it is in the environment around every forward"""

    def __init__(self, dev):
        self.dev, self.mods, self.full = dev, {}, {}

    def logits(self, name, fold, x, unfused="0"):
        import torch
        from clairs_to_amd import nn_shims
        old = {k: os.environ.get(k) for k in ("CTO_CVT_FOLD", "CTO_CVT_UNFUSED")}
        os.environ.update(CTO_CVT_FOLD=fold, CTO_CVT_UNFUSED=unfused)
        fold = fold + unfused                    # the module's key
        try:
            if (name, fold) not in self.mods:
                cfg, w = _config(name)[:2]
                m = (nn_shims.CvT if cfg["n_out"] == 4 else nn_shims.CvT_Indel)(model_type="acgt", **stage_kw(cfg)).eval()
                sd = m.state_dict()
                for k, v in w.items():
                    assert tuple(sd[k].shape) == v.shape, k
                    sd[k] = torch.from_numpy(v)
                m.load_state_dict(sd)
                self.mods[(name, fold)] = m
            got = self.mods[(name, fold)].logits(torch.from_numpy(np.ascontiguousarray(x)).to(self.dev)).cpu().numpy()
        finally:
            for k, v in old.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v
        assert np.isfinite(got).all(), (name, fold)
        return got

    def on_37(self, name, fold):
        if (name, fold) not in self.full:
            self.full[(name, fold)] = self.logits(name, fold, load_cvt_configs()[1])
        return self.full[(name, fold)]


@pytest.fixture(scope="module")
def paths(dev):
    return _Paths(dev)


@pytest.mark.parametrize("name", FOLDED)
def test_folded_path_is_as_close_to_fp64_as_the_unfolded_one(paths, name):
    _, _, l32, l64 = _config(name)
    fold, plain = paths.on_37(name, "1"), paths.on_37(name, "0")
    assert not np.array_equal(fold, plain), "CTO_CVT_FOLD selects nothing: both settings ran the same kernels"
    e_fold, e_plain = float(np.abs(fold - l64).max()), float(np.abs(plain - l64).max())
    e_ref = float(np.abs(l32.astype(np.float64) - l64).max())
    print("config %s: e_fold %.3g  e_plain %.3g  e_ref %.3g" % (name, e_fold, e_plain, e_ref))
    assert e_fold <= 2 * max(e_plain, e_ref), (name, e_fold, e_plain, e_ref)
    assert e_fold < BAR, (name, e_fold)


def test_generic_kernels_do_not_see_the_setting(paths):
    """F on the generic kernels in every stage (its stage 2, C = 72, has no other): the same bits under both settings"""
    x = load_cvt_configs()[1]
    np.testing.assert_array_equal(paths.logits("F", "1", x, unfused="1"), paths.logits("F", "0", x, unfused="1"))


@pytest.mark.parametrize("fold", ["1", "0"])
@pytest.mark.parametrize("name", FOLDED)
def test_tile_edges_give_the_bits_of_the_37_row_batch(paths, name, fold):
    """a site's logits do not depend on the batch it arrives in: 1 .. 33 sites (the golden rows repeated and truncated) against the
    same site in the 37-row batch on the same path, bit for bit; 1, 2 and 7 heads in stage 1 (C = 16 and 32), 3, 5 and 8 in stage 2"""
    x = load_cvt_configs()[1]
    full = paths.on_37(name, fold)
    for b in EDGES:
        idx = np.arange(b) % x.shape[0]
        np.testing.assert_array_equal(paths.logits(name, fold, x[idx]), full[:, idx], err_msg="config %s fold %s B %d" % (name, fold, b))
