"""cto_compare_calls on the device: equal - not close - to the host path of the same call and to the naive rules of comparevcfutil.py, at
record counts around the wave, the workgroup and scan.h's tile, with 0 to 3 BED sets; the running-count rule with the first SNV true
positive at either end; the sweep kernel around its tiles; the command on the device against the reference's files."""
import os

import numpy as np
import pytest

import calafutil
import comparevcfutil as u

pytestmark = pytest.mark.gpu

GOLDEN = u.golden()
CONFIGS = {c["name"]: c for c in GOLDEN["configs"]}


@pytest.mark.parametrize("n_sets", [0, 1, 2, 3])
@pytest.mark.parametrize("size", u.SIZES, ids=lambda s: "%dx%d" % s)
def test_device_equals_host_equals_naive(size, n_sets):
    """the seeded BED sets plant pos - 1 == start, == end - 1, == end and pos == start around the first records, a contig without intervals
    in a set that names others, a single-interval contig and (odd seed, three sets) a set that names none"""
    for seed in (0, 1):
        case = u.seeded_case(size[0], size[1], n_sets, seed)
        device, host = u.run_case(case, "device"), u.run_case(case, "host", host_threads=3)
        u.assert_same(device, host)
        u.assert_same(device, u.seeded_expected(size[0], size[1], n_sets, seed))


def test_membership_at_the_interval_ends():
    """one interval [10, 20) on contig 0, one contig the set does not name, a second set that names none"""
    pos = np.array([10, 11, 20, 21, 5, 11], dtype=np.int32)        # pos - 1: 9 out, 10 == start, 19 == end - 1, 20 == end, out, other contig
    n = len(pos)
    one = lambda v: np.full(n, v, dtype=np.int32)
    t = dict(ctg=np.array([0, 0, 0, 0, 0, 1], dtype=np.int32), pos=pos, ref_len=one(1), alt_len=one(1), n_alt=one(1), allele=one(0),
             gt=np.zeros((n, 2), dtype=np.int32), flags=np.zeros(n, dtype=np.uint8), qual=np.zeros(n))
    empty = dict((k, v[:0]) for k, v in t.items())
    beds1 = (np.array([1], dtype=np.int32), np.array([0, 1, 1], dtype=np.int64), np.array([10], dtype=np.int64), np.array([20], dtype=np.int64))
    beds2 = (np.array([1, 0], dtype=np.int32), np.array([0, 1, 1, 1, 1], dtype=np.int64), np.array([10], dtype=np.int64), np.array([20], dtype=np.int64))
    for beds, kept in ((beds1, [0, 1, 1, 0, 0, 0]), (beds2, [0] * 6)):
        case = dict(inp=t, tru=empty, beds=beds, n_ctg=2, benchmark_indel=False, high_confident_only=False, skip_genotyping=True, validate_phase=0,
                    cutoffs=np.zeros(0), roc_cutoffs=np.zeros(0))
        got = u.run_case(case, "device")
        np.testing.assert_array_equal((got["input_sets"] & u.KEPT) > 0, np.array(kept, dtype=bool))
        u.assert_same(got, u.naive(case))
        u.assert_same(got, u.run_case(case, "host"))
        swapped = dict(case, inp=empty, tru=dict((k, v) for k, v in t.items()))
        u.assert_same(u.run_case(swapped, "device"), u.naive(swapped))


@pytest.mark.parametrize("n", [300, 20000])
@pytest.mark.parametrize("snv_at", ["first", "last", None])
def test_running_count(n, snv_at):
    """20000 records take scan.h's three-launch form, 300 its one-workgroup form"""
    at = {"first": 0, "last": n - 1, None: None}[snv_at]
    case = u.running_count_case(n, at)
    got = u.run_case(case, "device")
    want = np.full(n, u.KEPT | u.TRUTH, dtype=np.uint8)
    if at is not None:
        want[at:] |= u.TP
    np.testing.assert_array_equal(got["input_sets"], want)
    u.assert_same(got, u.run_case(case, "host"))


@pytest.mark.parametrize("n_cut", [1, 64, 65, 101, 1000])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_sweep(n, n_cut):
    """values equal to a cut-off (>= against >), NaN values, negative values against the cut-off 0"""
    from clairs_to_amd.compare_vcf import sweep_counts
    values, sets, cutoffs = u.sweep_values(n, n_cut)
    got = sweep_counts(values, sets, cutoffs, where="device")
    np.testing.assert_array_equal(got, sweep_counts(values, sets, cutoffs, where="host"))
    v, s = (values, sets) if n * n_cut <= 500000 else (values[:400], sets[:400])       # the naive count is quadratic
    np.testing.assert_array_equal(sweep_counts(v, s, cutoffs, where="device"), u.naive_sweep(v.tolist(), s.tolist(), cutoffs.tolist()))
    if n:
        fp = values[(sets & u.FP) > 0]
        assert got[0, 0] == np.count_nonzero(fp >= 0.0)            # cut-off 0: -0.0 counts, -0.25 and NaN do not


def test_sweep_over_several_value_chunks():
    from clairs_to_amd.compare_vcf import sweep_counts
    values, sets, cutoffs = u.sweep_values(20001, 513)
    np.testing.assert_array_equal(sweep_counts(values, sets, cutoffs, where="device"), sweep_counts(values, sets, cutoffs, where="host"))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("compare_vcf_gpu"))
    u.write_inputs(d)
    return d


@pytest.mark.parametrize("name", ["demo", "bi_hc", "best_int", "roc", "minaf_bam"])
def test_the_command_on_the_device(files, tmp_path, capsys, name):
    from clairs_to_amd.__main__ import dispatch
    cf = CONFIGS[name]
    seen = {}
    for where in ("device", "host"):
        out = tmp_path / where
        out.mkdir()
        capsys.readouterr()
        dispatch("compare_vcf", u.config_argv(cf, files, out, where, bam=calafutil.case()["bam"] if "@BAM@" in cf["argv"] else None))
        written = {}
        for base, _, fs in os.walk(str(out)):
            for f in fs:
                written[os.path.relpath(os.path.join(base, f), str(out))] = open(os.path.join(base, f)).read()
        seen[where] = (capsys.readouterr().out, written)
    assert seen["device"] == seen["host"]
    assert seen["device"] == (cf["stdout"], cf["files"])
