"""The CvT forward (clairs/model.py:57-147, 231-261) in numpy float64, batched: an fp64 yardstick for configurations whose golden file
holds the reference's fp32 logits only (tests/golden/models_CvT.npz).  test_cvt_fp64.py checks it against the reference's own fp64
runs of configurations A and B (tests/golden/models_CvT_configs.npz)."""
import math

import numpy as np

_HEADS = ("a", "c", "g", "t", "i", "d")
_erf = np.vectorize(math.erf, otypes=[np.float64])


def _selu(a):
    scale, alpha = 1.0507009873554804934193349852946, 1.6732632423543772848170429916717
    return np.where(a > 0, scale * a, scale * alpha * np.expm1(np.minimum(a, 0.0)))


def _chan_ln(x, g, b):
    """the reference's channel LayerNorm: eps is added to the standard deviation; x [B, W, C]"""
    m = x.mean(-1, keepdims=True)
    sd = np.sqrt(((x - m) ** 2).mean(-1, keepdims=True))
    return (x - m) / (sd + 1e-5) * g.reshape(-1) + b.reshape(-1)


def _dw_bn(y, stride, w, P):
    """depth-wise 3-tap conv (middle row of the 3x3 kernel, pad 1) + BatchNorm(eval); y [B, W, C]"""
    dw = w[P + ".net.0.weight"].astype(np.float64)[:, 0, 1, :]        # [C, 3]
    yp = np.pad(y, ((0, 0), (1, 1), (0, 0)))
    W = y.shape[1]
    s = sum(yp[:, t:t + W] * dw[:, t] for t in range(3))[:, ::stride]
    f = lambda n: w[P + ".net.1." + n].astype(np.float64)
    return (s - f("running_mean")) / np.sqrt(f("running_var") + 1e-5) * f("weight") + f("bias")


def cvt_forward_fp64(w, cfg, x):
    """w: state_dict name -> array; cfg = dict(emb_dim, heads, depth, n_out); x [B, 33, 34] -> logits [K, B, 2] float64"""
    h = np.asarray(x, dtype=np.float64)
    f = lambda n: w[n].astype(np.float64)
    for s in range(3):
        C, heads = cfg["emb_dim"][s], cfg["heads"][s]
        L = "layer%d" % (s + 1)
        cw = f(L + ".0.weight")[:, :, 1, :]                            # [C, Cin, 3]: only kernel row 1 meets the height-1 map
        W = h.shape[1]
        Wo = (W + 1) // 2
        hp = np.pad(h, ((0, 0), (1, 1), (0, 0)))
        t = f(L + ".0.bias") + sum(hp[:, tp:tp + 2 * Wo:2] @ cw[:, :, tp].T for tp in range(3))
        h = _chan_ln(t, f(L + ".1.g"), f(L + ".1.b"))
        for d in range(cfg["depth"][s]):
            P = "%s.2.layers.%d" % (L, d)
            y = _chan_ln(h, f(P + ".0.norm.g"), f(P + ".0.norm.b"))
            q = _dw_bn(y, 1, w, P + ".0.fn.to_q") @ f(P + ".0.fn.to_q.net.2.weight").reshape(64 * heads, C).T
            kv = _dw_bn(y, 2, w, P + ".0.fn.to_kv") @ f(P + ".0.fn.to_kv.net.2.weight").reshape(128 * heads, C).T
            B, Wkv = kv.shape[0], kv.shape[1]
            qh = q.reshape(B, Wo, heads, 64).transpose(0, 2, 1, 3)
            kh = kv[..., :64 * heads].reshape(B, Wkv, heads, 64).transpose(0, 2, 1, 3)
            vh = kv[..., 64 * heads:].reshape(B, Wkv, heads, 64).transpose(0, 2, 1, 3)
            dots = qh @ kh.transpose(0, 1, 3, 2) * 0.125
            e = np.exp(dots - dots.max(-1, keepdims=True))
            o = ((e / e.sum(-1, keepdims=True)) @ vh).transpose(0, 2, 1, 3).reshape(B, Wo, 64 * heads)
            h = h + o @ f(P + ".0.fn.to_out.0.weight").reshape(C, 64 * heads).T + f(P + ".0.fn.to_out.0.bias")
            y = _chan_ln(h, f(P + ".1.norm.g"), f(P + ".1.norm.b"))
            u = y @ f(P + ".1.fn.net.0.weight").reshape(4 * C, C).T + f(P + ".1.fn.net.0.bias")
            u = 0.5 * u * (1.0 + _erf(u / math.sqrt(2.0)))
            h = h + u @ f(P + ".1.fn.net.3.weight").reshape(C, 4 * C).T + f(P + ".1.fn.net.3.bias")
    feat = h.transpose(0, 2, 1).reshape(h.shape[0], -1)                # torch flattens [C][1][W] as c * W + w
    g = _selu(feat @ f("fc1.weight").T + f("fc1.bias"))
    out = []
    for k in range(cfg["n_out"]):
        u = _selu(g @ f(_HEADS[k] + "_fc2.weight").T + f(_HEADS[k] + "_fc2.bias"))
        out.append(_selu(u @ f(_HEADS[k] + "_fc3.weight").T + f(_HEADS[k] + "_fc3.bias")))
    return np.stack(out)
