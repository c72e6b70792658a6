"""The realigner's fast pass on its own results (cto_fast_pass_batch, host form; csrc/realign.cpp: Window::fast_pass_host): every
haplotype's score and every (haplotype, read) hit's score and start against a plain model of the order-dependent rules
(tests/fastpassutil.model), integer for integer, on windows built for the rules' edges - each test asserts from the model's trace
that the case it is named for occurred.  End to end the same windows give what the compiled reference returned
(tests/golden/realign_fastpass.json.gz).  tests/test_gpu_fast_pass.py holds k_fast_pass to the same."""
import numpy as np
import pytest

import fastpassutil as fp
import realignutil as ru


@pytest.mark.parametrize("family", sorted(fp.FAMILIES))
def test_host_fast_pass_equals_the_model(family):
    """lengths: L = 32, 33; reads of 32, 33, L, L + 5.  start0: a tandem repeat opens the haplotype, the start-0 hit is visited on a
    clipped diagonal first.  ties: equal scores at several starts, the first visited wins.  mismatches_and_n: 2 against 3; N in the
    read, the haplotype, both.  coverage_rule: dropped; prefix beyond; suffix = L; suffix = L + 50 (the bound wraps); the reference.
    visit_time: every seeded position covered in the end, one not yet when it is tested.  degenerate: a read twice, none, short ones."""
    fp.check_family(family, ["host"])


def test_host_fast_pass_on_fresh_windows():
    """300 windows of a fresh seed (L 32 .. 200, repeats, overhanging reads, prefix and suffix up to L + 50): host form = model; where
    oracle/_ref is built, POS and CIGAR of these windows are the compiled reference's as well"""
    seed, ws, ms = fp.fresh_windows()
    fp.check_fresh_traces(ms)
    got = fp.run(ws, "host", threads=4)
    for i, (g, (m, _)) in enumerate(zip(got, ms)):
        assert fp.same(g, m), "window %d of np.random.default_rng(%d): host %s model %s" % (i, seed, fp.triple_lists(g), fp.triple_lists(m))
    if ru.ref_lib() is None:
        return
    out = ru.amd_realign_batch(ws, "host", threads=4)
    for i, (w, o) in enumerate(zip(ws, out)):
        assert tuple(o) == tuple(ru.ref_realign(w)), "window %d of np.random.default_rng(%d)" % (i, seed)


def test_host_fast_pass_at_the_device_limits():
    """FP_LMAX - 1, FP_LMAX x FP_RMAX - 1, FP_RMAX, unique sequence: reads on diagonal 0 and on the last diagonal, 2 mismatches taken, 3 not"""
    lim = fp.limits()
    names = sorted(fp.limit_cases(lim))
    assert len(names) == 4
    for k in names:
        w, m, tr = fp.fixed()[k]
        L, R = len(w["haplotypes"][1]), len(w["seqs"][0])
        assert m[2][1].tolist() == [0, -1, (L - R) // 2 - 7, L - R] and m[1][1].tolist() == [4 * R, 0, 4 * (R - 2) - 12, 4 * (R - 1) - 6]
        assert tr["seeded_rejected"] > 0 and tr["dropped"] == 0 and tr["kept_scoring"] == 2
        assert fp.same(fp.run([w], "host")[0], m), k


def test_host_fast_pass_on_the_candidate_list_windows():
    """FP_CAND - 1, FP_CAND, FP_CAND + 1 and 3 x FP_CAND listed diagonals per (haplotype, read) - counted by the model -, one of them with
    an accepted hit, one with seeds and no acceptance"""
    lim = fp.limits()
    for k, (n, w) in fp.candidate_cases(lim).items():
        _, m, tr = fp.fixed()[k]
        assert tr["listed"] == [[n, n], [n, n]] and tr["accepted"] == 4 and tr["seeded_rejected"] >= 4, (k, tr)
        assert fp.same(fp.run([w], "host")[0], m), k


def test_host_fast_pass_batch_layout():
    """(H, reads) = (1, 1), (18, 3), (2, 0), (3, 60) in one call, in reverse order, cut in two: the same triples"""
    ws = fp.layout_cases()
    assert [(len(w["haplotypes"]), len(w["seqs"])) for w in ws] == [(1, 1), (18, 3), (2, 0), (3, 60)]
    ms = [fp.fixed()["layout_%d" % i][1] for i in range(4)]
    assert sum(int((m[1] > 0).sum()) for m in ms) >= 10
    names = ["layout_%d" % i for i in range(4)]
    fp.assert_equal_to_model(names, ws, fp.run(ws, "host"), ms, "host")
    fp.assert_equal_to_model(names[::-1], ws[::-1], fp.run(ws[::-1], "host", threads=3), ms[::-1], "host, reversed")
    fp.assert_equal_to_model(names, ws, fp.run(ws[:2], "host") + fp.run(ws[2:], "host"), ms, "host, cut in two")


def test_fixed_windows_end_to_end_on_the_host_equal_the_compiled_reference():
    """POS and CIGAR of every fixed window through cto_realign_windows (host) = what the reference's realigner returned (stored)"""
    want = fp.golden_outputs()
    names = sorted(want)
    assert set(names) == set(fp.fixed()) and sum(len(v[0]) for v in want.values()) > 100
    got = ru.amd_realign_batch([fp.fixed()[k][0] for k in names], "host", threads=4)
    for k, g in zip(names, got):
        assert tuple(g) == tuple(want[k]), k
        if ru.ref_lib() is not None and fp.fixed()[k][0]["seqs"]:
            assert tuple(g) == tuple(ru.ref_realign(fp.fixed()[k][0])), k


def test_fast_pass_entry_points():
    """the limits come from the library; no jobs is no output; a window of the host's size is fine on the host; mismatched outputs are refused"""
    from clairs_to_amd._lib import lib, RealignJob
    lim = fp.limits()
    assert set(lim) == {"FP_LMAX", "FP_RMAX", "FP_CAND", "FP_NT"} and all(v > 0 for v in lim.values())
    assert lim["FP_NT"] % 64 == 0 and lim["FP_RMAX"] > fp.K and lim["FP_LMAX"] >= lim["FP_RMAX"]
    assert fp.run([], "host") == []
    rng = np.random.default_rng(3)
    ref = fp.rs(rng, lim["FP_LMAX"] + 1)
    w = fp.window([ref[5:5 + lim["FP_RMAX"] + 1]], [5], ref, [ref], 10, 10)
    (hs, sc, ps), = fp.run([w], "host")
    assert hs.tolist() == [4 * (lim["FP_RMAX"] + 1)] and ps.tolist() == [[5]]
    jobs = (RealignJob * 1)()
    jobs[0].n_reads, jobs[0].reference, jobs[0].haplotypes = 0, b"A" * 40, b"A" * 40 + b" " + b"C" * 40
    out = np.zeros(4, dtype=np.int32)
    assert lib.cto_fast_pass_batch(1, jobs, 0, 1, None, out.ctypes.data, 1, None, None, 0, None) != 0       # two haplotypes, room for one
    assert lib.cto_fast_pass_batch(1, jobs, 0, 1, None, out.ctypes.data, 2, None, None, 0, None) == 0
    assert lib.cto_fast_pass_batch(1, jobs, 7, 1, None, out.ctypes.data, 2, None, None, 0, None) != 0
