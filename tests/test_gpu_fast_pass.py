"""k_fast_pass (csrc/realign_batch.hip) on its own results, through cto_fast_pass_batch: every haplotype's score and every (haplotype,
read) hit's score and start from the kernel = from the host form = from the plain model of the order-dependent rules
(tests/fastpassutil.model), integer for integer - at the rules' edges (what finish() never shows: hits on haplotypes that are not
picked, scores that do not change the order, haplotypes the coverage rule drops), at the kernel's limits FP_LMAX x FP_RMAX, around
the capacity FP_CAND of its list of diagonals, and across the layouts of a batch.  With where = "device" the entry refuses what the
kernel does not take, so every call that returns ran the kernel."""
import numpy as np
import pytest

import fastpassutil as fp
import realignutil as ru

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


def pairs_of(ws):
    return sum(len(w["haplotypes"]) * len(w["seqs"]) for w in ws)


@pytest.mark.parametrize("family", sorted(fp.FAMILIES))
def test_device_fast_pass_equals_the_host_form_and_the_model(dev, family):
    """the families of tests/test_fast_pass.py::test_host_fast_pass_equals_the_model, kernel and host form against the model"""
    fp.check_family(family, ["device", "host"])
    ws = [fp.fixed()[k][0] for k in fp.FAMILIES[family]]
    st = {}
    fp.run(ws, "device", stats=st)
    assert st["fast_pairs"] == pairs_of(ws) and st["windows"] == len(ws) and st["host_windows"] == 0


def test_device_fast_pass_on_fresh_windows(dev):
    """300 windows of a fresh seed: kernel = host form = model; end to end on the device the compiled reference's POS and CIGAR where
    oracle/_ref is built, the host's otherwise"""
    seed, ws, ms = fp.fresh_windows()
    fp.check_fresh_traces(ms)
    st = {}
    d, h = fp.run(ws, "device", threads=8, stats=st), fp.run(ws, "host", threads=8)
    assert st["fast_pairs"] == pairs_of(ws)
    for i, (a, b, (m, _)) in enumerate(zip(d, h, ms)):
        assert fp.same(a, m) and fp.same(b, m), "window %d of np.random.default_rng(%d): device %s host %s model %s" % (
            i, seed, fp.triple_lists(a), fp.triple_lists(b), fp.triple_lists(m))
    st = {}
    out = ru.amd_realign_batch(ws, "device", threads=8, stats=st)
    assert st["host_windows"] == 0 and st["fast_pairs"] == pairs_of(ws)
    want = ru.amd_realign_batch(ws, "host", threads=8) if ru.ref_lib() is None else [ru.ref_realign(w) for w in ws]
    for i, (o, r) in enumerate(zip(out, want)):
        assert tuple(o) == tuple(r), "window %d of np.random.default_rng(%d)" % (i, seed)


def test_fixed_windows_end_to_end_on_the_device_equal_the_compiled_reference(dev):
    """POS and CIGAR of every fixed window through cto_realign_windows on the device = the reference's (stored) = the host's"""
    want = fp.golden_outputs()
    names = sorted(want)
    ws = [fp.fixed()[k][0] for k in names]
    st = {}
    got = ru.amd_realign_batch(ws, "device", threads=8, stats=st)
    assert st["host_windows"] == 0 and st["fast_pairs"] == pairs_of(ws)
    host = ru.amd_realign_batch(ws, "host", threads=8)
    for k, g, h in zip(names, got, host):
        assert tuple(g) == tuple(want[k]) and tuple(h) == tuple(want[k]), k


def test_device_fast_pass_at_its_limits(dev):
    """L in {FP_LMAX - 1, FP_LMAX} x reads of {FP_RMAX - 1, FP_RMAX}: ten trips of the workgroup over the diagonals, the last one partly
    filled; reads on diagonal 0 and on the last one.  One base more - the reference, a haplotype, a read - sends exactly that window to
    the host inside cto_realign_windows, and cto_fast_pass_batch refuses it on the device."""
    from clairs_to_amd._lib import CtoError
    lim = fp.limits()
    LM, RM = lim["FP_LMAX"], lim["FP_RMAX"]
    names = sorted(fp.limit_cases(lim))
    ws, ms = [fp.fixed()[k][0] for k in names], [fp.fixed()[k][1] for k in names]
    assert (LM - fp.K) + (RM - fp.K) + 1 > 9 * lim["FP_NT"] and [len(w["haplotypes"][1]) for w in ws] == [LM - 1, LM - 1, LM, LM]
    fp.assert_equal_to_model(names, ws, fp.run(ws, "device"), ms, "device")
    fp.assert_equal_to_model(names, ws, fp.run(ws, "host"), ms, "host")
    rng = np.random.default_rng(11)
    small = fp.fixed()["two_against_three"][0]
    ref = fp.rs(rng, LM)
    hap = fp.sub(ref, 700)
    reads, at = [hap[600:600 + 150], fp.sub(hap[650:650 + RM], 9), hap[:RM]], [600, 650, 0]
    over = {
        "reference": fp.window(reads, at, ref + "A", [hap, ref], 50, 50),
        "haplotype": fp.window(reads, at, ref, [ref, hap + "C"], 50, 50),
        "read": fp.window(reads + [hap[100:100 + RM + 1]], at + [100], ref, [ref, hap], 50, 50),
    }
    for what, w in over.items():
        st = {}
        got = ru.amd_realign_batch([small, w, small], "device", threads=4, stats=st)
        assert st["host_windows"] == 1 and st["windows"] == 3, what
        assert got == ru.amd_realign_batch([small, w, small], "host", threads=4), what
        assert all(c != g for c, g in zip(w["cigars"], got[1][1])), what             # placed by the fast pass: 'X', not the input's 'M'
        assert fp.same(fp.run([w], "host")[0], fp.model(w)[0]), what
        with pytest.raises(CtoError, match="window 1"):
            fp.run([small, w, small], "device")
    st = {}
    inside = fp.window(reads, at, ref, [ref, hap], 50, 50)
    ru.amd_realign_batch([inside], "device", stats=st)
    assert st["host_windows"] == 0


def test_device_fast_pass_around_the_capacity_of_its_candidate_list(dev):
    """FP_CAND - 1, FP_CAND, FP_CAND + 1 and 3 x FP_CAND listed diagonals (the model's count): which of them wavefronts walk and which the
    threads that found them is a race the result must not depend on - three runs, one result, the host's and the model's"""
    lim = fp.limits()
    for k, (n, w) in fp.candidate_cases(lim).items():
        _, m, tr = fp.fixed()[k]
        assert tr["listed"] == [[n, n], [n, n]] and tr["accepted"] == 4 and tr["seeded_rejected"] >= 4, (k, tr)
        runs = [fp.run([w], "device")[0] for _ in range(3)]
        for g in runs:
            assert fp.same(g, m), "%s: device %s model %s" % (k, fp.triple_lists(g), fp.triple_lists(m))
        assert fp.same(fp.run([w], "host")[0], m), k


def test_device_fast_pass_batch_layout(dev):
    """(H, reads) = (1, 1), (18, 3), (2, 0), (3, 60) in one call, in reverse order, cut in two: hit_off, hap_win, win_read0"""
    ws = fp.layout_cases()
    names = ["layout_%d" % i for i in range(4)]
    ms = [fp.fixed()[k][1] for k in names]
    st = {}
    fp.assert_equal_to_model(names, ws, fp.run(ws, "device", stats=st), ms, "device")
    assert st["fast_pairs"] == 1 + 54 + 0 + 180 and st["haplotypes"] == 24 and st["reads"] == 64
    fp.assert_equal_to_model(names[::-1], ws[::-1], fp.run(ws[::-1], "device", threads=3), ms[::-1], "device, reversed")
    fp.assert_equal_to_model(names, ws, fp.run(ws[:2], "device") + fp.run(ws[2:], "device"), ms, "device, cut in two")
    fp.assert_equal_to_model(names[2:3], ws[2:3], fp.run(ws[2:3], "device"), ms[2:3], "device, the window without reads alone")
    assert fp.run([], "device") == []
