"""The k/v-side form of the folded attention weights (csrc/cvt_block.h: FOLD_KV; DESIGN.md 7.1 "Folded onto the k/v rows"), selected
with CTO_CVT_FOLD=kv in every fused geometry, against the unfolded kernels (CTO_CVT_FOLD=0), the q-side form (CTO_CVT_FOLD=q) and the
fp64 runs of the reference network, on the 37 golden rows of cvtconfigutil.py:

  S  16,64,128 / 1,3,4 / 1,2,3 / 4   the default SNV configuration: stage 3 with 4 heads, three blocks + embedding + classifier in one launch
  A  16,64,128 / 2,5,8 / 4,5,1 / 4   stage 3 with 8 heads as ONE block; stage 2 with 5 heads, 4 + 1 blocks; stage 1 (C = 16), four blocks
  B  32,64,128 / 7,8,2 / 2,1,5 / 6   stage 3 with 2 heads, 4 + 1 blocks (the classifier in a launch without embedding); stage 2 with 8
                                     heads; stage 1 at C = 32 (eight lanes per query row) with 7 heads
  F  16,72,128 / 7,3,4 / 1,2,3 / 6   stage 2 at C = 72 has no fused kernel: stage 3 behind the GEMM embedding; stage 1 with 7 heads

Since this form exists, stage 3 (C = 128) is folded too: the sentence "stage 3 (C = 128 > dim_head) never is" in
test_gpu_cvt_fold.py's docstring describes the q-side form alone.  That file's tests compare the default against CTO_CVT_FOLD=0 and
hold unchanged.

The bound is that file's: one product with a matrix formed in double and rounded once replaces two rounded products (k' = ykv Mq^T
for q and k; v' = ykv Mo for v and the out-projection) - the same order of error, not provably smaller - so this form may sit at most
twice as far from fp64 as the worse of the unfolded path and the fp32 reference, and under the project's 1e-4 bar.

max |logit - fp64| over the 37 rows on an MI355X, CTO_CVT_FOLD=kv / =0 / the fp32 reference:
    S  1.45e-05 / 1.43e-05 / 5.94e-06
    A  1.30e-05 / 1.28e-05 / 6.35e-06
    B  2.26e-05 / 3.42e-05 / 1.01e-05
    F  1.42e-05 / 2.31e-05 / 9.96e-06
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_models_npz
from cvt_fp64 import cvt_forward_fp64
from cvtconfigutil import BAR, load_cvt_configs, stage_kw, weights_of
from weights_recipe import CVT_CFG, make_weights

pytestmark = pytest.mark.gpu

CONFIGS = ("S", "A", "B", "F")
EDGES = (1, 7, 8, 9, 15, 16, 17, 33)         # around the 8- and 16-site tiles, ragged last tiles, more than one workgroup
_refs = {}


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _config(name):
    """(cfg with n_out, recipe weights, logits32 [K,37,2], logits64 [K,37,2]) of a configuration on the 37 rows, computed once"""
    if name not in _refs:
        cfgs, x = load_cvt_configs()
        if name != "S":
            c = cfgs[name]
            _refs[name] = (c["cfg"], weights_of(name), c["logits32"], c["logits64"])
        else:
            g = load_models_npz("CvT")
            rows = np.load(os.path.join(GOLDEN, "models_CvT_configs.npz"))["rows"]
            cfg, w = dict(CVT_CFG, n_out=g["n_out"]), make_weights(g["manifest"], seed=g["n_out"])
            _refs[name] = (cfg, w, g["logits"][:, rows], cvt_forward_fp64(w, cfg, x))
    return _refs[name]


class _Paths:
    """one module per (configuration, CTO_CVT_FOLD, CTO_CVT_UNFUSED) and its logits on the 37 rows, computed once; the settings are read
    when a handle is created and CTO_CVT_FOLD is part of the shim's handle key, so both are in the environment around every forward"""

    def __init__(self, dev):
        self.dev, self.mods, self.full = dev, {}, {}

    def logits(self, name, fold, x, unfused="0"):
        import torch
        from clairs_to_amd import nn_shims
        old = {k: os.environ.get(k) for k in ("CTO_CVT_FOLD", "CTO_CVT_UNFUSED")}
        os.environ.update(CTO_CVT_FOLD=fold, CTO_CVT_UNFUSED=unfused)
        key = (name, fold, unfused)
        try:
            if key not in self.mods:
                cfg, w = _config(name)[:2]
                m = (nn_shims.CvT if cfg["n_out"] == 4 else nn_shims.CvT_Indel)(model_type="acgt", **stage_kw(cfg)).eval()
                sd = m.state_dict()
                for k, v in w.items():
                    assert tuple(sd[k].shape) == v.shape, k
                    sd[k] = torch.from_numpy(v)
                m.load_state_dict(sd)
                self.mods[key] = m
            got = self.mods[key].logits(torch.from_numpy(np.ascontiguousarray(x)).to(self.dev)).cpu().numpy()
        finally:
            for k, v in old.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v
        assert np.isfinite(got).all(), key
        return got

    def on_37(self, name, fold):
        if (name, fold) not in self.full:
            self.full[(name, fold)] = self.logits(name, fold, load_cvt_configs()[1])
        return self.full[(name, fold)]


@pytest.fixture(scope="module")
def paths(dev):
    return _Paths(dev)


@pytest.mark.parametrize("name", CONFIGS)
def test_kv_side_form_is_as_close_to_fp64_as_the_unfolded_one(paths, name):
    _, _, l32, l64 = _config(name)
    kv, plain = paths.on_37(name, "kv"), paths.on_37(name, "0")
    e_kv, e_plain = float(np.abs(kv - l64).max()), float(np.abs(plain - l64).max())
    e_ref = float(np.abs(l32.astype(np.float64) - l64).max())
    print("config %s: e_kv %.3g  e_plain %.3g  e_ref %.3g" % (name, e_kv, e_plain, e_ref))
    assert e_kv <= 2 * max(e_plain, e_ref), (name, e_kv, e_plain, e_ref)
    assert e_kv < BAR, (name, e_kv)


def test_each_setting_selects_kernels_of_its_own(paths):
    """kv, q and 0 run three different sets of kernels on S: no two give the same bits"""
    got = {f: paths.on_37("S", f) for f in ("kv", "q", "0")}
    for a, b in (("kv", "q"), ("kv", "0"), ("q", "0")):
        assert not np.array_equal(got[a], got[b]), "CTO_CVT_FOLD=%s and =%s ran the same kernels" % (a, b)


def test_generic_kernels_do_not_see_the_setting(paths):
    """F on the generic kernels in every stage: the same bits under kv and 0"""
    x = load_cvt_configs()[1]
    np.testing.assert_array_equal(paths.logits("F", "kv", x, unfused="1"), paths.logits("F", "0", x, unfused="1"))


@pytest.mark.parametrize("name", CONFIGS)
def test_tile_edges_give_the_bits_of_the_37_row_batch(paths, name):
    """a site's logits do not depend on the batch it arrives in: 1 .. 33 sites (the golden rows repeated and truncated) against the
    same site in the 37-row batch, bit for bit - the pad rows of the 48- and 80-row k/v tiles (72 of 80 in stage 1), ragged last tiles,
    and the sums over heads that a query row keeps in registers, which must never pick up a neighbour's row"""
    x = load_cvt_configs()[1]
    full = paths.on_37(name, "kv")
    for b in EDGES:
        idx = np.arange(b) % x.shape[0]
        np.testing.assert_array_equal(paths.logits(name, "kv", x[idx]), full[:, idx], err_msg="config %s B %d" % (name, b))
