"""cvt_fp64.py is a faithful fp64 CvT: it reproduces the fp64 runs of the REFERENCE's own modules stored for configurations A and B
(tests/golden/models_CvT_configs.npz) to rounding, and sits as close to the reference's fp32 logits of the default SNV configuration
(tests/golden/models_CvT.npz) as an fp32 run sits to an fp64 one.  test_gpu_cvt_fold.py takes its fp64 logits of that configuration,
for which the golden file holds fp32 logits only, from it."""
import numpy as np
import pytest

from conftest import load_models_npz
from cvt_fp64 import cvt_forward_fp64
from cvtconfigutil import load_cvt_configs, weights_of
from weights_recipe import CVT_CFG, make_weights


@pytest.mark.parametrize("name", ["A", "B"])
def test_fp64_forward_reproduces_the_reference_fp64_run(name):
    cfgs, x = load_cvt_configs()
    c = cfgs[name]
    got = cvt_forward_fp64(weights_of(name), c["cfg"], x)
    # two fp64 evaluations of the same network in different summation orders: 1e-11 is 1e5 times what they differ by in
    # relative terms at logits of order 1 and 1e5 times below the fp32 reference's own error (5e-6)
    assert np.abs(got - c["logits64"]).max() < 1e-11


def test_fp64_forward_of_the_default_configuration_sits_at_the_fp32_reference():
    g = load_models_npz("CvT")
    got = cvt_forward_fp64(make_weights(g["manifest"], seed=g["n_out"]), dict(CVT_CFG, n_out=g["n_out"]), g["x"])
    assert np.abs(got - g["logits"]).max() < 2e-5        # the fp32 reference is 5e-6 .. 1e-5 from fp64 on the seven configurations
