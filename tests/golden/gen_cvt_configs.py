"""CvT configurations off the two the other fixtures pin: the reference's own modules at other widths, head counts and depths.

Run in the build container only (imports /root/reference):   python tests/golden/gen_cvt_configs.py
Writes tests/golden/models_CvT_configs.npz = data only:
  configs            JSON: [[name, emb_dim x3, heads x3, depth x3, n_out], ...]
  rows               [37] indices into models_CvT.npz's x (np.random.default_rng(5).integers(0, len(x), 37)); the rows
                     themselves are not stored again
  per configuration <n> in A .. G:
    manifest_<n>     JSON [(state_dict name, shape)] of the reference module built with those keywords
    logits32_<n>     [K,37,2]  clairs.model.CvT (K = 4) / CvT_Indel (K = 6) in eval(), fp32, torch CPU, 1 thread, filled
                     with make_weights(manifest, seed=K)
    logits64_<n>     [K,37,2]  the SAME module after .double()
What each configuration reaches in the HIP engine is tabulated in tests/cvtconfigutil.py.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, HERE)
from weights_recipe import make_weights  # noqa: E402

# name, emb_dim, heads, depth, n_out
CONFIGS = (("A", (16, 64, 128), (2, 5, 8), (4, 5, 1), 4),
           ("B", (32, 64, 128), (7, 8, 2), (2, 1, 5), 6),
           ("C", (20, 48, 100), (2, 5, 8), (2, 1, 4), 4),
           ("D", (4, 128, 12), (8, 1, 2), (1, 1, 1), 4),
           ("E", (128, 16, 32), (1, 1, 1), (1, 1, 1), 6),
           ("F", (16, 72, 128), (7, 3, 4), (1, 2, 3), 6),
           ("G", (8, 24, 4), (3, 6, 4), (1, 1, 2), 6))
N_ROWS = 37


def main():
    sys.path.insert(0, REF)
    import torch
    import clairs.model as rm
    torch.set_num_threads(1)
    base = np.load(os.path.join(HERE, "models_CvT.npz"))["x"]
    rows = np.random.default_rng(5).integers(0, len(base), N_ROWS)
    x = torch.from_numpy(base[rows])
    out = dict(rows=rows.astype(np.int64), configs=json.dumps([[n, list(e), list(h), list(d), k] for n, e, h, d, k in CONFIGS]))
    for name, emb, heads, depth, n_out in CONFIGS:
        kw = dict(num_classes=2, apply_softmax=False, model_type="acgt")
        for i in range(3):
            kw.update({"s%d_emb_dim" % (i + 1): emb[i], "s%d_heads" % (i + 1): heads[i], "s%d_depth" % (i + 1): depth[i]})
        m = (rm.CvT if n_out == 4 else rm.CvT_Indel)(**kw)
        manifest = [(k, list(v.shape)) for k, v in m.state_dict().items() if not k.endswith("num_batches_tracked")]
        w = make_weights(manifest, seed=n_out)
        sd = m.state_dict()
        for k, v in w.items():
            sd[k] = torch.from_numpy(v.copy())
        m.load_state_dict(sd)
        m.eval()
        with torch.no_grad():
            l32 = np.stack([o.numpy() for o in m(x)])
            l64 = np.stack([o.numpy() for o in m.double()(x.double())])
        assert l32.shape == (n_out, N_ROWS, 2) and l64.dtype == np.float64
        out["manifest_" + name] = json.dumps(manifest)
        out["logits32_" + name] = l32.astype(np.float32)
        out["logits64_" + name] = l64
        print("%s emb %-14s heads %-10s depth %-10s K %d: %7d parameters, max|logit| %5.2f, ref32 vs ref64 %.3g" % (
            name, emb, heads, depth, n_out, sum(int(np.prod(s)) for _, s in manifest), np.abs(l64).max(),
            np.abs(l32 - l64).max()))
    np.savez_compressed(os.path.join(HERE, "models_CvT_configs.npz"), **out)


if __name__ == "__main__":
    main()
