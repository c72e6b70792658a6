"""What the CvT configuration tests share: tests/golden/models_CvT_configs.npz (gen_cvt_configs.py) and its recipe weights.

Configurations, as emb / heads / depth / K, and what each reaches in the HIP engine (csrc/models.hip, cvt_block.h, nn_kernels.h):
  A  16,64,128 / 2,5,8 / 4,5,1 / 4   fused kernels with 2, 5 and 8 heads; one full group of CVT_MAX_BLK = 4 blocks; 4 + 1; stage 3 as
                                     ONE block that carries the embedding and the classifier tail
  B  32,64,128 / 7,8,2 / 2,1,5 / 6   fused C = 32 with 7 heads; stage-3 depth 4 + 1: the tail in a one-block launch without embedding
  C  20,48,100 / 2,5,8 / 2,1,4 / 4   generic kernels in all stages: C % 16 != 0, C % 16 == 0 without a kernel; conv K = 60, 144;
                                     fc1 K = 500 (four K slices of 128, the last one ragged)
  D  4,128,12  / 8,1,2 / 1,1,1 / 4   the smallest width; stage-1 k_attention at 8 heads (76 576 B of LDS); the N <= 16 GEMM shape;
                                     C = 128 off its geometry; fc1 K = 60 (slices of 16, the last one ragged)
  E  128,16,32 / 1,1,1 / 1,1,1 / 6   stage 1 at C = 128 (k_ln_dw's s_y full, k_layernorm's second element per lane); conv K = 384, 48;
                                     fc1 K = 160
  F  16,72,128 / 7,3,4 / 1,2,3 / 6   fused stage 1 with 7 heads, generic stage 2 at 72, fused stage 3 behind a GEMM embedding with
                                     K = 216, fused tail
  G  8,24,4    / 3,6,4 / 1,1,2 / 6   fc1 K = 20: kslice = 16, so two of the four K slices are EMPTY (kbeg >= K); N = 24 on the
                                     64-wide GEMM shape; conv K = 24, 72
"""
import json
import os

import numpy as np

from conftest import GOLDEN
from weights_recipe import make_weights

NAMES = ("A", "B", "C", "D", "E", "F", "G")
BAR = 1e-4           # the project's model bar (test_gpu_parity.py: test_models_match_reference_logits)

_cache = {}


def load_cvt_configs():
    """{name: dict(cfg, n_out, manifest, logits32, logits64)}, the 37 input rows, read once"""
    if not _cache:
        z = np.load(os.path.join(GOLDEN, "models_CvT_configs.npz"))
        x = np.load(os.path.join(GOLDEN, "models_CvT.npz"))["x"][z["rows"]]
        cfgs = {}
        for name, emb, heads, depth, n_out in json.loads(str(z["configs"])):
            cfgs[name] = dict(cfg=dict(emb_dim=tuple(emb), heads=tuple(heads), depth=tuple(depth), n_out=n_out), n_out=n_out,
                              manifest=[(k, tuple(s)) for k, s in json.loads(str(z["manifest_" + name]))],
                              logits32=z["logits32_" + name], logits64=z["logits64_" + name])
        _cache["v"] = (cfgs, np.ascontiguousarray(x, dtype=np.float32))
    return _cache["v"]


def weights_of(name):
    """the recipe weights of a configuration (seed = K, as the generator filled the reference's module); shared, do not modify"""
    key = "w" + name
    if key not in _cache:
        c = load_cvt_configs()[0][name]
        _cache[key] = make_weights(c["manifest"], seed=c["n_out"])
    return _cache[key]


def stage_kw(cfg):
    """the s{1,2,3}_{emb_dim,heads,depth} keywords of clairs.model.CvT / nn_shims.CvT"""
    kw = {}
    for i in range(3):
        kw.update({"s%d_emb_dim" % (i + 1): cfg["emb_dim"][i], "s%d_heads" % (i + 1): cfg["heads"][i],
                   "s%d_depth" % (i + 1): cfg["depth"][i]})
    return kw
