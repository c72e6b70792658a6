"""What tests/test_bigru_layers.py (CPU) and tests/test_gpu_bigru_layers.py (device) share: the two recurrent layers of the BiGRU and
the fc1 partial sums the fused layer-2 kernel leaves behind (csrc/gru_kernel.h, csrc/gru_split_kernel.h), stated three times -

  * `torch_layer` / `fc1_partials`: torch.nn.GRU(bidirectional=True, batch_first=True), the module clairs/model.py:412-417 itself uses,
    in float64 (the reference) and in float32 (the "twin": its distance from the float64 run on the same inputs and weights is the
    unit in which a kernel's distance is judged, `BARS`);
  * `np_layer` / `np_partials`: the same recurrence in plain numpy, with switchable DEFECTS - the slips a kernel of this shape can
    make - so that the CPU test can show that each of them moves something the device test looks at by far more than its bar;
  * `tile_ranges`: the launch rule of csrc/gru_tiles.h, from which the device test derives the batch shapes that reach each path.

Selector fc1 sets: fc1.weight one-hot, so that output n of the slab of direction d IS one element (t, j) of layer 2's state of that
direction - the only window onto a state the kernel never writes out."""
import numpy as np

from conftest import load_models_npz, load_range_npz
from weights_recipe import make_weights

T, C, H1, H2, NF = 33, 34, 128, 192, 128
N_SELECTORS = 6

# How many times the float32 twin's own distance from float64 a kernel may sit from float64: twice the worst multiple measured on
# MI355X, rounded up (the measured figures: module docstring of tests/test_gpu_bigru_layers.py).  Keys: (kernel, weight scale), then
# quantity - "h1" layer 1's output, "h2" layer 2's state as the selector sets show it, "slab" the dense fc1 partial sums.
BARS = {
    ("f32", 1): {"h1": 4, "h2": 5, "slab": 16},
    ("f32", 3): {"h1": 3, "h2": 4, "slab": 10},
    ("f16", 1): {"h1": 12, "h2": 2, "slab": 8},
    ("bf16", 1): {"h1": 188, "h2": 26, "slab": 23},
}
# the fp32 kernels must not need more than this (beyond it the distance is a finding to explain, not a bar to set)
FP32_CEILING = 16


# ---------------------------------------------------------------- launch rule
def tile_ranges(cus, B):
    """[(begin, end, sites per tile)] of a batch of B on a part with `cus` compute units (csrc/gru_tiles.h)"""
    rnd = 16 * cus
    full, rest = B // rnd * rnd, B % rnd
    out = [(0, full, 32)] if full else []
    return out + ([(full, B, 32 if 4 * rest > 3 * rnd else 16)] if rest else [])


def geometry_shapes(cus):
    """name -> (B, the ranges it is meant to run as)"""
    rnd = 16 * cus
    q = 3 * rnd // 4
    return {
        "last16": (q, [(0, q, 16)]),
        "first32": (q + 1, [(0, q + 1, 32)]),
        "ragged32": (q + 29, [(0, q + 29, 32)]),
        "second16": (rnd + 17, [(0, rnd, 32), (rnd, rnd + 17, 16)]),
        "second32": (rnd + q + 29, [(0, rnd, 32), (rnd, rnd + q + 29, 32)]),
        "two_rounds": (2 * rnd + 1, [(0, 2 * rnd, 32), (2 * rnd, 2 * rnd + 1, 16)]),
    }


def sample_rows(cus, B, n_max=128, seed=0):
    """the rows of a batch that go to the host: the first tiles' edges, every row of the last tile of each range, the rows around each
    range's begin, the last row, and random rows up to n_max in all"""
    rows = {r for r in (0, 15, 16, 31, 32, B - 1) if 0 <= r < B}
    for begin, end, th in tile_ranges(cus, B):
        rows |= set(range(begin + (end - begin - 1) // th * th, end))
        rows |= {r for r in (begin - 1, begin) if 0 <= r < B}
    assert len(rows) <= n_max
    rest = np.setdiff1d(np.arange(B), sorted(rows))
    extra = np.random.default_rng(seed).choice(rest, size=min(len(rest), n_max - len(rows)), replace=False)
    return np.sort(np.concatenate([np.array(sorted(rows), dtype=np.int64), extra.astype(np.int64)]))


# ---------------------------------------------------------------- inputs and weights
def fixture_windows():
    """[97][33][34] float32: the 45 golden windows and the 52 of the range fixture (unrescaled depth 8 000, all-zero, one-hot, x 1/1024)"""
    return np.concatenate([load_models_npz("BiGRU_NACGT")["x"], load_range_npz("BiGRU_NACGT")["x"]]).astype(np.float32)


def resampled_windows(n, seed=1):
    """n windows drawn from the 97, each times its own factor from U(0.5, 1.5): no two rows of a batch are equal"""
    w = fixture_windows()
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, len(w), size=n)
    f = rng.uniform(0.5, 1.5, size=n)
    assert len(np.unique(f)) == n
    return (w[idx].astype(np.float64) * f[:, None, None]).astype(np.float32)


def recipe_weights(cls="BiGRU_NACGT", scale=1.0):
    g = load_models_npz(cls)
    return make_weights(g["manifest"], seed=g["n_out"], scale=scale)


def selector_map(s):
    """(t, j) [2][128] of selector set s: which element of layer 2's state output n of direction d's slab shows.  Sets 0-4 walk the
    640 observations q = 128 s + n over j = q mod 192 and over every step (steps 0 and 32 first); set 5 shows again what sets 0-4
    show, at other outputs (so in other waves and lanes of the kernel): output n repeats output 127 - n of set n mod 5."""
    n = np.arange(NF)
    if s == N_SELECTORS - 1:
        src = [selector_map(k) for k in range(N_SELECTORS - 1)]
        return np.stack([np.stack([src[i % 5][d][:, 127 - i] for i in n], axis=1) for d in range(2)])
    q = NF * s + n
    t0 = np.where(q < 64, (q % 2) * (T - 1), (5 * q + q // 192) % T)
    j0 = q % H2
    return np.stack([np.stack([t0, j0]), np.stack([(T - 1 - t0 + 7 * (q // 64)) % T, (H2 - 1 - j0 + 64 * s) % H2])])


def selector_fc1(s):
    """fc1.weight [128][33 * 384] of selector set s"""
    m = selector_map(s)
    w = np.zeros((NF, T, 2, H2), dtype=np.float32)
    for d in range(2):
        w[np.arange(NF), m[d][0], d, m[d][1]] = 1.0
    return w.reshape(NF, T * 2 * H2)


def selector_pick(h2, s):
    """what the slabs of selector set s must hold: [2][B][128] out of h2 [B][33][384]"""
    m = selector_map(s)
    return np.stack([h2[:, m[d][0], d * H2 + m[d][1]] for d in range(2)])


# ---------------------------------------------------------------- torch reference
def torch_layer(w, name, x, dtype):
    """layer `name` ("lstm" / "lstm_2") on x [B][33][K] in `dtype` on the CPU -> numpy [B][33][2H] of that dtype"""
    import torch
    H = H1 if name == "lstm" else H2
    gru = torch.nn.GRU(x.shape[2], H, num_layers=1, batch_first=True, bidirectional=True)
    gru.load_state_dict({k[len(name) + 1:]: torch.as_tensor(np.asarray(v)) for k, v in w.items() if k.startswith(name + ".")})
    gru = gru.to(dtype).eval()
    with torch.no_grad():
        return gru(torch.as_tensor(np.asarray(x)).to(dtype))[0].numpy()


def fc1_partials(h2, fc1w):
    """slab[d][b][n] = sum_t sum_j h2[b][t][d 192 + j] fc1w[n][t 384 + d 192 + j], in h2's dtype"""
    B = h2.shape[0]
    f = np.asarray(fc1w, dtype=h2.dtype).reshape(NF, T, 2, H2)
    h = h2.reshape(B, T, 2, H2)
    return np.stack([h[:, :, d].reshape(B, T * H2) @ f[:, :, d].reshape(NF, T * H2).T for d in range(2)])


# ---------------------------------------------------------------- numpy restatement with defects
DEFECTS = ("swap_bias_n", "swap_rz", "h_lag", "drop_last_channel", "drop_chunk", "drop_chunk_one_row", "last_step", "reverse_fc1_shift",
           "neighbour_row")
DEFECT_CHUNK, DEFECT_GATE, DEFECT_UNIT, DEFECT_SITE = 5, 2, 77, 17      # the k-chunk dropped; gate (n) and unit of the single row; the tile row


def _sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def np_direction(x, w_ih, w_hh, b_ih, b_hh, reverse, defect=None):
    """one direction of torch.nn.GRU (gates r, z, n) in float64: [B][33][K] -> [B][33][H]"""
    x = np.asarray(x, dtype=np.float64)
    w_ih, w_hh, b_ih, b_hh = (np.array(a, dtype=np.float64) for a in (w_ih, w_hh, b_ih, b_hh))
    B, H = x.shape[0], w_hh.shape[1]
    if defect == "swap_bias_n":
        b_ih[2 * H:], b_hh[2 * H:] = b_hh[2 * H:].copy(), b_ih[2 * H:].copy()
    if defect == "drop_last_channel":
        w_ih[:, -1] = 0.0
    if defect == "drop_chunk":
        w_hh[:, 16 * DEFECT_CHUNK:16 * DEFECT_CHUNK + 16] = 0.0
    if defect == "drop_chunk_one_row":
        w_hh[DEFECT_GATE * H + DEFECT_UNIT, 16 * DEFECT_CHUNK:16 * DEFECT_CHUNK + 16] = 0.0
    if defect == "neighbour_row" and B > DEFECT_SITE + 1:
        x = x.copy()
        x[DEFECT_SITE] = x[DEFECT_SITE + 1]
    out = np.zeros((B, T, H))
    h = h_before = np.zeros((B, H))
    for step in range(T):
        t = T - 1 - step if reverse else step
        gi = x[:, t] @ w_ih.T + b_ih
        gh = (h_before if defect == "h_lag" else h) @ w_hh.T + b_hh
        r = _sigmoid(gi[:, :H] + gh[:, :H])
        z = _sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        if defect == "swap_rz":
            r, z = z, r
        n = np.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        h_before, h = h, (1.0 - z) * n + z * h
        if not (defect == "last_step" and step == T - 1):       # the last step's state never leaves the kernel
            out[:, t] = h
    return out


def np_layer(w, name, x, defect=None):
    """both directions of layer `name`, float64 [B][33][2H]"""
    return np.concatenate([np_direction(x, w[name + ".weight_ih_l0" + sfx], w[name + ".weight_hh_l0" + sfx], w[name + ".bias_ih_l0" + sfx],
                                        w[name + ".bias_hh_l0" + sfx], sfx != "", defect) for sfx in ("", "_reverse")], axis=2)


def np_partials(h2, fc1w, defect=None):
    """fc1_partials in float64; reverse_fc1_shift: the reverse direction's state of step t meets the fc1 slice of step t + 1"""
    h2 = np.asarray(h2, dtype=np.float64)
    if defect == "reverse_fc1_shift":
        h2 = h2.copy()
        h2[:, 1:, H2:] = h2[:, :-1, H2:].copy()
        h2[:, 0, H2:] = 0.0
    return fc1_partials(h2, np.asarray(fc1w, dtype=np.float64))
