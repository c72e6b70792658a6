"""The column kernels at the depth and key counts the engine allows (csrc/pack_internal.h: 32 767 read-bases and 2 048 distinct indel
keys per column): k_featurize_sites and k_featurize_columns count two passes in the 16-bit halves of one word and hand int16 on,
k_extract_candidates keeps four 16-bit counters in one register, the entry word gives the key id 11 bits - so the limits have to be
exact, and the paths only deep or key-rich columns reach (the unstaged extraction walk, the first-seen overflow pass, further key
sweeps) have to give what the others give.  The reference is the CPU oracle on mpileup text written from the same arrays; the one-kernel
and the two-stage featurisation are compared with each other in addition.  Everything is integer and bit-exact.

One window (33 or 34 columns, one or two candidates) per case; the over-limit inputs live in test_deep_columns.py and never reach
a kernel."""
import types

import numpy as np
import pytest

import columnutil as cu

pytestmark = pytest.mark.gpu

SWEEP = ["depth201", "depth4097", "depth8000", "depth32767", "mixed"]
COMPOSITION = ["fwd_ref", "fwd_alt", "rev_alt", "low_bq", "low_mq", "one_insertion", "star", "split"]
KEYS = ["keys257", "keys2048"]
LATE = ["late_indels"]        # 32 767 read-bases whose last 200 carry indels: few enough for the device tokeniser's single pass
ALT_STRIDE = 1 << 18          # the alt_info of 2 048 keys is longer than the oracle wrapper's default row


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _build(name):
    """-> (chunk, run-list columns or None, candidate positions)"""
    from clairs_to_amd.synth import SynthChunk
    if name.startswith("depth"):
        # every column of x-16 .. x+17 at depth D, the generator's composition; the second candidate's window is the other 33 columns
        d = int(name[5:])
        ch = SynthChunk(1, seed=20261019 + d, p_ins=0.02, p_del=0.02, depth=d)
        return ch, None, [int(ch.site_pos[0]), int(ch.site_pos[0]) + 1]
    if name == "mixed":
        depth = np.full(34, 4)
        depth[16] = cu.LIMIT
        ch = SynthChunk(1, seed=20261020, p_ins=0.02, p_del=0.02, depth=depth)
        return ch, None, [int(ch.site_pos[0])]
    if name in COMPOSITION:
        cols = cu.window(cu.POS, cu.composition_cases()[name][0])
    elif name in KEYS:
        cols = cu.window(cu.POS, cu.key_edge_runs(int(name[4:])))
    elif name in LATE:
        keys = [(cu.A, 1, (2, 1)), (cu.c, 1, (3, 0)), (cu.A, 2, (4, 0)), (cu.g, 2, (1, 0)), (cu.STAR, 1, (5, 2))]
        runs = [(cu.A, 0, 40, 60, None, cu.LIMIT - 200)] + [keys[i % 5][:2] + (40 if i % 3 else 10, 60, keys[i % 5][2], 1) for i in range(200)]
        cols = cu.window(cu.POS, runs)
    else:
        assert name == "gates"
        cols = cu.gate_columns()[0]
        return cu.run_chunk(cols, [cols[0][0] + 16]), cols, [cols[0][0] + 16]
    return cu.run_chunk(cols, [cu.POS]), cols, [cu.POS]


@pytest.fixture(scope="module")
def win(request, dev):
    """One window, built once for all the tests that ask for it: the chunk, its NEG-pass text, the host pack of that text (which must
    be the chunk's own arrays) and the arrays in HBM."""
    import oracle
    from clairs_to_amd.pack import ColumnPack, DevicePack
    oracle.build()
    name = request.param
    ch, cols, sites = _build(name)
    w = types.SimpleNamespace(name=name, chunk=ch, cols=cols, sites=np.asarray(sites, dtype=np.int32))
    w.ref, w.lo = ch.ref_window()
    w.text0 = oracle.synth_mpileup_text(ch, 0)
    w.pack = ColumnPack.from_mpileup(w.text0, w.ref, w.lo)
    got, want = w.pack.numpy(), ch.arrays()
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    w.dp = DevicePack(want, dev)
    cache = {}

    def tensor_of(q):
        if q not in cache:
            text = w.text0 if q == 0 else oracle.synth_mpileup_text(ch, q)
            cache[q] = oracle.create_tensor(text, w.ref, w.lo, w.sites, alt_stride=ALT_STRIDE)
        return cache[q]
    w.oracle_tensor = tensor_of
    return w


def _featurize_both(w, dev, min_bq, rescale):
    import torch
    from clairs_to_amd.featurize import featurize
    sp = torch.from_numpy(w.sites).to(dev)
    two = featurize(w.dp, sp, min_bq, rescale, want_raw=True, fused=False)
    one = featurize(w.dp, sp, min_bq, rescale, want_raw=True, fused=True)
    torch.cuda.synchronize()
    return one, two


def _check_against_oracle(w, feat, min_bq, rescale, oracle_lib, tag):
    from clairs_to_amd.featurize import alt_infos
    info = feat.site_info.cpu().numpy()
    np.testing.assert_array_equal(w.chunk.col_pos[info[:, 0]], w.sites, err_msg=tag)
    for pass_idx, q, raw, x in ((0, min_bq, feat.raw_aff, feat.x_aff), (1, 0, feat.raw_neg, feat.x_neg)):
        t, depth, alts, flags = w.oracle_tensor(q)
        np.testing.assert_array_equal(info[:, 3] & 1, flags, err_msg=tag)
        np.testing.assert_array_equal(raw.cpu().numpy().astype(np.int32), t, err_msg="%s pass %d" % (tag, pass_idx))
        np.testing.assert_array_equal(info[:, 1 + pass_idx], depth, err_msg=tag)
        np.testing.assert_array_equal(x.cpu().numpy(), oracle_lib.rescale(t, depth, rescale), err_msg=tag)      # bit-exact fp32
        assert alt_infos(feat, w.pack, info, pass_idx=pass_idx) == alts, "%s pass %d alt_info" % (tag, pass_idx)
        if pass_idx == 0:
            f, r = oracle_lib.strand_counts(t)
            np.testing.assert_array_equal(info[:, 4:8], f, err_msg=tag)
            np.testing.assert_array_equal(info[:, 8:12], r, err_msg=tag)


def _check_one_equals_two(w, one, two, dev):
    import torch
    for name in ("x_aff", "x_neg", "raw_aff", "raw_neg", "site_info", "sitefirst"):
        assert torch.equal(getattr(one, name), getattr(two, name)), name
    centre = two.site_info[:, 0].long()
    assert torch.equal(one.site_colvec, two.colvec.index_select(0, centre))
    ko = w.chunk.key_off.astype(np.int64)
    keys = np.concatenate([np.arange(ko[c], ko[c + 1]) for c in centre.cpu().tolist()] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    if keys.size:
        kt = torch.from_numpy(keys).to(dev)
        assert torch.equal(one.keycnt.index_select(0, kt), two.keycnt.index_select(0, kt))
        assert torch.equal(one.keyfirst.index_select(0, kt), two.keyfirst.index_select(0, kt))


@pytest.mark.parametrize("win", SWEEP + COMPOSITION + KEYS + LATE, indirect=True)
def test_featurisation_at_depth_matches_the_oracle(win, dev, oracle_lib):
    """Both featurisation paths against the oracle - tensors of both passes, depths, skip flags, strand counts, rescaled inputs and the
    alt_info strings (key counts and first-seen order) - and against each other, at --min_bq 20 with rescale 50 and at --min_bq 0
    without rescale."""
    if win.name.startswith("depth"):
        d = int(win.name[5:])
        assert (np.diff(win.chunk.col_off) == d).all() and win.chunk.col_pos.size == 34
    for min_bq, rescale in ((20, 50), (0, 0)):
        one, two = _featurize_both(win, dev, min_bq, rescale)
        _check_against_oracle(win, one, min_bq, rescale, oracle_lib, "%s one kernel min_bq %d" % (win.name, min_bq))
        _check_against_oracle(win, two, min_bq, rescale, oracle_lib, "%s two stages min_bq %d" % (win.name, min_bq))
        _check_one_equals_two(win, one, two, dev)


@pytest.mark.parametrize("win", COMPOSITION, indirect=True)
def test_a_full_column_of_one_kind_fills_its_channels_and_no_other(win, dev):
    """32 767 read-bases of one kind in the candidate column: the channels written down by hand in columnutil.composition_cases hold
    +-32 767 (or the 16 384 / 16 383 split) and every other channel of the column is zero, in both passes and both paths."""
    _, want, depth = cu.composition_cases()[win.name]
    one, two = _featurize_both(win, dev, 20, 0)
    for tag, feat in (("one kernel", one), ("two stages", two)):
        info = feat.site_info.cpu().numpy()
        for p, raw in ((0, feat.raw_aff), (1, feat.raw_neg)):
            col = raw.cpu().numpy()[0, cu.FLANK].astype(np.int64)
            got = {int(i): int(col[i]) for i in np.nonzero(col)[0]}
            assert got == want[p], (win.name, tag, p)
            assert info[0, 1 + p] == depth[p], (win.name, tag, p)
        # the neighbours: four forward reference bases each
        rest = np.delete(feat.raw_neg.cpu().numpy()[0].astype(np.int64), cu.FLANK, axis=0)
        assert (np.abs(rest).sum(axis=1) == 4).all() and (rest.min(axis=1) == -4).all()
    if win.name == "low_bq":           # AFF 0 beside NEG 32 767: the packed counter word was 0x7fff0000
        cv = one.site_colvec.cpu().numpy()[0].astype(np.int64)
        assert cv[1] == 0 and cv[36 + 1] == cu.LIMIT


@pytest.mark.parametrize("win", KEYS, indirect=True)
def test_key_rich_candidate_column(win, dev):
    """257 and 2 048 distinct indel keys in a 4 096-deep candidate column (more than the 256 first-seen slots of LDS, several key
    sweeps): every key's two counts and two first-seen indices against a count over the run list, on both paths."""
    runs = win.cols[cu.FLANK][2]
    want = cu.expected_keys(runs, 20)
    nk = int(win.name[4:])
    assert want.shape[0] == nk and len(runs) == 4096
    assert (want[:, 2] != want[:, 3]).sum() > nk // 8, "keys the two passes first meet at different read-bases"
    assert ((want[:, 2] == 0x7fffffff) & (want[:, 3] != 0x7fffffff)).any() and ((want[256:, 3] > 4000) & (want[256:, 3] < 4096)).any()
    c = cu.FLANK
    k0, k1 = int(win.chunk.key_off[c]), int(win.chunk.key_off[c + 1])
    assert k1 - k0 == nk and int((win.chunk.entries[win.chunk.col_off[c]:win.chunk.col_off[c + 1]] >> 21).max()) == nk - 1
    one, two = _featurize_both(win, dev, 20, 50)
    for tag, feat in (("one kernel", one), ("two stages", two)):
        cnt = feat.keycnt.cpu().numpy().view(np.uint32)[k0:k1].astype(np.int64)
        first = feat.keyfirst.cpu().numpy()[k0:k1].astype(np.int64)
        np.testing.assert_array_equal(cnt & 0xffff, want[:, 0], err_msg=tag)
        np.testing.assert_array_equal(cnt >> 16, want[:, 1], err_msg=tag)
        np.testing.assert_array_equal(first[:, 0], want[:, 2], err_msg=tag)
        np.testing.assert_array_equal(first[:, 1], want[:, 3], err_msg=tag)


def _check_extraction(w, dev, oracle_lib, params, select_indel, by_hand=None, hybrid=True):
    from clairs_to_amd.extract_candidates_calling import extract_candidates, candidate_positions, hybrid_info_rows
    snv_af, indel_af, cov, abn = params
    ch = w.chunk
    text6 = oracle_lib.synth_mpileup_text(ch, 20, None, 20, False)
    pos, fl, dep = oracle_lib.extract_candidates(text6, w.ref, w.lo, snv_af, indel_af, cov, abn, select_indel)
    flags, depth = extract_candidates(w.dp, 20, 20, snv_af, indel_af, cov, abn, select_indel)
    got_f, got_d = flags.cpu().numpy(), depth.cpu().numpy()
    cols = np.searchsorted(ch.col_pos, pos)                        # rows exist only where some read passes the MQ gate
    tag = "%s %r select_indel %d" % (w.name, params, select_indel)
    np.testing.assert_array_equal(got_f[cols], fl, err_msg=tag)
    np.testing.assert_array_equal(got_d[cols], dep, err_msg=tag)
    mask = np.ones(ch.col_pos.size, bool)
    mask[cols] = False
    assert not got_f[mask].any(), tag
    for bit in (1, 2):
        assert candidate_positions(w.dp, flags, bit).cpu().tolist() == pos[(fl & bit) != 0].tolist(), tag
    if hybrid:
        want_rows = oracle_lib.hybrid_info_rows(text6, w.ref, w.lo, ch.col_pos, "chr1", snv_af, indel_af, cov, abn, select_indel)
        assert hybrid_info_rows(w.pack, w.dp, flags, ch.col_pos, "chr1", 20, 20, select_indel) == want_rows, tag
    if by_hand:
        at = {int(p): int(f) for p, f in zip(pos, fl)}
        for p, (snv, indel) in by_hand.items():
            assert (at[p] & 1, (at[p] >> 1) & 1) == (snv, indel if select_indel else 0), (tag, p)
    return got_f


@pytest.mark.parametrize("select_indel", [True, False])
@pytest.mark.parametrize("win", SWEEP + COMPOSITION + KEYS, indirect=True)
def test_extraction_at_depth_matches_the_oracle(win, dev, oracle_lib, select_indel):
    """k_extract_candidates (staged below 4 096 read-bases per 64 columns, unstaged above; its four 16-bit counters per register),
    the candidate lists and the hybrid-info rows of every column of the window against the oracle on the extraction pileup."""
    # the key-rich columns carry deletions longer than max_indel_length, whose per-allele hybrid-info row is CTO_EUNSUPPORTED by design
    f = _check_extraction(win, dev, oracle_lib, (0.05, 0.05, 4, 3), select_indel, hybrid=win.name not in KEYS)
    if win.name in ("fwd_alt", "rev_alt", "split", "mixed"):
        assert f[cu.FLANK] & 1, "the candidate column is an SNV candidate"


@pytest.mark.parametrize("select_indel", [True, False])
@pytest.mark.parametrize("win", ["gates"], indirect=True)
def test_extraction_gates_at_depth(win, dev, oracle_lib, select_indel):
    """Columns exactly on the AF, read-count and coverage gates at depths around 32 760, and 20 merged indel alleles in a 32 767-deep
    column (more than the 16 a lane counts in LDS): the oracle, and the side of each gate written down by hand."""
    for params, by_hand in cu.gate_columns()[1]:
        _check_extraction(win, dev, oracle_lib, params, select_indel, by_hand)


@pytest.mark.parametrize("win", ["depth8000", "depth32767"] + LATE, indirect=True)
def test_device_tokeniser_at_depth(win, dev, record_property):
    """The text of a deep window through cto_tokenise_device: the pack of the host tokeniser, whether the single pass took the rows
    or declined them to the host (either is in the contract; which one is reported)."""
    from clairs_to_amd.pack import DeviceTokeniser
    tok = DeviceTokeniser()                      # the arrays of a result live in the context
    got = tok(win.text0, win.ref, win.lo)
    path = "declined to the host" if got is None else "tokenised on the device"
    record_property("tokeniser_path", path)
    print("device tokeniser, %s: %s" % (win.name, path))
    if got is not None:
        view, lite = got
        a, b = win.pack.numpy(), DeviceTokeniser.download(view)
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        assert (lite.n_cols, lite.n_keys) == (win.pack.n_cols, win.pack.n_keys)


@pytest.mark.parametrize("K", [4, 6])
@pytest.mark.parametrize("win", ["fwd_ref", "fwd_alt"], indirect=True)
def test_raw_inputs_at_the_int16_extremes(win, dev, K):
    """cto_model_forward_raw on tensors that hold -32 767 and +32 767, rescale on: the logits of the fp32 hand-over, bit for bit
    (test_gpu_raw_inputs.py at the ends of the int16 range), both networks."""
    import torch
    from clairs_to_amd._lib import lib, check
    from clairs_to_amd.engine import Engine, synthetic_models
    from clairs_to_amd.featurize import featurize
    from clairs_to_amd.synth import likelihood_table, lik_and_edges
    models = synthetic_models(K)
    lik, edges = lik_and_edges(likelihood_table(K), K)
    eng = Engine(models["aff"], models["neg"], lik, edges, device=dev)
    sp = torch.from_numpy(win.sites).to(dev)
    feat = featurize(win.dp, sp, 20, 50, want_raw=True, want_x=True)
    raw = feat.raw_aff.cpu().numpy()
    assert abs(int(raw.min())) == cu.LIMIT and (win.name == "fwd_ref" or int(raw.max()) == cu.LIMIT)
    s = int(torch.cuda.current_stream().cuda_stream)
    B = int(sp.numel())
    for handle, which in ((eng.h_aff, 0), (eng.h_neg, 1)):
        out_raw, out_x = torch.empty((K, B, 2), device=dev), torch.empty((K, B, 2), device=dev)
        x = feat.raw_aff if which == 0 else feat.raw_neg
        check(lib.cto_model_forward_raw(handle, x.data_ptr(), feat.site_info.data_ptr(), which, 50, B, out_raw.data_ptr(), s))
        x = feat.x_aff if which == 0 else feat.x_neg
        check(lib.cto_model_forward(handle, x.data_ptr(), B, out_x.data_ptr(), s))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out_raw.cpu().numpy(), out_x.cpu().numpy(), err_msg="%s which %d" % (win.name, which))
        assert torch.isfinite(out_raw).all()
