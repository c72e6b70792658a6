"""get_logr_and_baf and predict_germline_genotypes (steps 2 and 4 of the reference's Verdict chain) against what the reference wrote on the
same inputs (tests/golden/verdict_gg.json.gz, written by tests/golden/gen_verdict_gg.py): every argv through the dispatch of
`python -m clairs_to_amd`, byte for byte - predict_germline_genotypes through the host path of cto_germline_window_dist; that path's
distances, on arrays freshly seeded every run, against a short plain-numpy restatement of the three medians; the chain from an
alleleCounter-format table to the genotype table."""
import os
import random

import numpy as np
import pytest

import verdictsim
from conftest import load_json_gz


@pytest.fixture(scope="module")
def golden():
    return load_json_gz("verdict_gg.json.gz")


def write_files(d, files):
    for k, v in files.items():
        with open(os.path.join(d, k), "w") as f:
            f.write(v)


def run_and_compare(sub, run, extra):
    from clairs_to_amd.__main__ import dispatch
    dispatch(sub, list(run["argv"]) + extra)
    assert run["outputs"]
    for fn, text in run["outputs"].items():
        assert open(fn).read() == text, (run["name"], fn)
        os.remove(fn)


def restated_dist(c, segment_length):
    """the rules of the issue, in plain numpy, for one run"""
    m = len(c)
    if m <= 5:
        return np.ones(m)
    L = min(m - 1, segment_length)
    H = L // 2
    out = np.full(m, np.inf)
    for k in range(m):
        medians = []
        if k >= L:
            medians.append(np.median(c[k - L:k]))
        if k < m - L:
            medians.append(np.median(c[k + 1:k + L + 1]))
        if H <= k < m - H:
            medians.append(np.median(np.concatenate((c[k - H:k], c[k + 1:k + H + 1]))))
        if medians:
            out[k] = min(np.abs(md - c[k]) for md in medians)
    return out


def fresh_runs(rng, ms):
    """runs of mirrored BAFs as the tables hold them (alt / depth, depths of 200 - 400, some values repeated) and their offsets"""
    cs = []
    for m in ms:
        depth = rng.integers(200, 401, size=m)
        alt = rng.binomial(depth, 0.5) if rng.random() < 0.7 else rng.integers(0, 4, size=m) * (depth // 8)
        baf = alt / depth
        cs.append(np.where(baf < 0.5, baf, 1 - baf))
    return np.concatenate(cs) if cs else np.zeros(0), np.concatenate(([0], np.cumsum(ms))).astype(np.int64)


def same_bits(a, b):
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


def test_both_names_are_submodules():
    from clairs_to_amd.__main__ import SUBMODULES
    assert "get_logr_and_baf" in SUBMODULES and "predict_germline_genotypes" in SUBMODULES


def test_the_python_constants_are_the_header_s():
    import re
    from clairs_to_amd import predict_germline_genotypes as pgg
    from conftest import ROOT
    header = open(os.path.join(ROOT, "include", "clairsto_amd.h")).read()
    assert int(re.search(r"#define CTO_GG_TILE\s+(\d+)", header).group(1)) == pgg.GG_TILE
    assert int(re.search(r"#define CTO_GG_MAX_SEGMENT\s+(\d+)", header).group(1)) == pgg.GG_MAX_SEGMENT >= 100


def test_get_logr_and_baf_byte_for_byte(golden, tmp_path, monkeypatch):
    g = golden["counts"]
    files = verdictsim.count_files(g["spec"])
    assert verdictsim.digest(files) == g["inputs_sha256"]
    write_files(str(tmp_path), files)
    monkeypatch.chdir(tmp_path)
    assert [r["name"] for r in g["runs"]] == ["tumour_only", "with_normal"]
    for run in g["runs"]:
        assert len(run["outputs"]) == (3 if run["name"] == "with_normal" else 2)
        run_and_compare("get_logr_and_baf", run, ["--seed", str(run["seed"])])


def test_get_logr_and_baf_without_a_seed_draws_from_the_clock(golden, tmp_path, monkeypatch):
    """no --seed: the seed is int(time()), as the reference's on import"""
    from clairs_to_amd import get_logr_and_baf
    g = golden["counts"]
    write_files(str(tmp_path), verdictsim.count_files(g["spec"]))
    monkeypatch.chdir(tmp_path)
    run = g["runs"][0]
    monkeypatch.setattr(get_logr_and_baf, "time", lambda: run["seed"] + 0.75)
    run_and_compare("get_logr_and_baf", run, [])


@pytest.fixture(scope="module")
def gg_files(golden):
    files = verdictsim.baf_files(golden["gg"]["spec"])
    assert verdictsim.digest(files) == golden["gg"]["inputs_sha256"]
    return files


def test_predict_germline_genotypes_byte_for_byte_on_the_host_path(golden, gg_files, tmp_path, monkeypatch):
    write_files(str(tmp_path), gg_files)
    monkeypatch.chdir(tmp_path)
    names = [r["name"] for r in golden["gg"]["runs"]]
    assert names == ["defaults", "segment7", "segment2", "no_extra_hetero", "max_homozygous", "normal_baf"]
    for run in golden["gg"]["runs"]:
        run_and_compare("predict_germline_genotypes", run, ["--where", "host"])


def test_the_cut_is_strict_in_every_tumour_only_scenario(golden, gg_files):
    """equal distances across the cut would leave the choice to numpy's unstable argsort: the fixture must not depend on it"""
    from clairs_to_amd.predict_germline_genotypes import undecided_runs, window_dist
    rows = [r.split("\t") for r in gg_files["baf.txt"].split("\n")[1:] if r]
    baf = np.array([r[2] for r in rows]).astype(float)
    bsm = np.where(baf < 0.5, baf, 1 - baf)
    n_cut = 0
    for run in golden["gg"]["runs"]:
        if run["cut"] is None:
            continue
        opt = dict(zip(run["argv"][::2], run["argv"][1::2]))
        limit = max(np.sort(bsm)[round(len(bsm) * 0.65)], float(opt.get("--maxHomozygous", 0.02)))
        undecided = ~(bsm < limit)
        assert int(undecided.sum()) == run["cut"]["undecided"]
        st = {}
        dist = window_dist(bsm[undecided], undecided_runs([r[0] for r in rows], undecided), int(opt.get("--segmentLength", 100)), "host", st)
        assert st["host_path"] == 1 and st["n_probes"] == len(dist)
        s, e = np.sort(dist), run["cut"]["extra_hetero"]
        assert s[e - 1] < s[e], run["name"]
        assert (repr(float(s[e - 1])), repr(float(s[e]))) == (run["cut"]["below"], run["cut"]["above"]), run["name"]
        assert int(np.isinf(dist).sum()) == run["cut"]["infinite"]
        n_cut += 1
    assert n_cut == 4
    assert next(r for r in golden["gg"]["runs"] if r["name"] == "defaults")["cut"]["infinite"] >= 1
    # the spec's undecided counts are the ones the issue lists, the tile run included
    from clairs_to_amd.predict_germline_genotypes import GG_TILE
    ms = [m for _, m in golden["gg"]["spec"]["runs"]]
    assert set((0, 1, 5, 6, 7, 12, 101, 102, 300, 2 * GG_TILE + 3)) <= set(ms)
    names = [c for c, _ in golden["gg"]["spec"]["runs"]]
    assert len(set(names)) < len(names)                        # a chromosome name comes back


def test_segment_length_below_two_is_refused(gg_files, tmp_path, monkeypatch):
    from clairs_to_amd.__main__ import dispatch
    from clairs_to_amd._lib import CtoError
    from clairs_to_amd.predict_germline_genotypes import window_dist
    write_files(str(tmp_path), gg_files)
    monkeypatch.chdir(tmp_path)
    argv = ["--tumor_logr_file", "logr.txt", "--tumor_baf_file", "baf.txt", "--germline_genotypes_output_file", "out.txt", "--where", "host"]
    with pytest.raises(SystemExit) as e:
        dispatch("predict_germline_genotypes", argv + ["--segmentLength", "1"])
    assert "segmentLength" in str(e.value)
    assert not os.path.exists("out.txt")
    with pytest.raises(CtoError):
        window_dist(np.full(8, 0.4), [0, 8], 1, "host")


def test_a_missing_logr_file_raises(gg_files, tmp_path, monkeypatch):
    from clairs_to_amd.__main__ import dispatch
    write_files(str(tmp_path), gg_files)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(FileNotFoundError):
        dispatch("predict_germline_genotypes", ["--tumor_logr_file", "nowhere.txt", "--tumor_baf_file", "baf.txt", "--germline_genotypes_output_file", "out.txt",
                                                "--where", "host"])


def test_bad_input_is_an_error_of_the_c_call():
    from clairs_to_amd._lib import CtoError
    from clairs_to_amd.predict_germline_genotypes import window_dist
    c = np.full(20, 0.4)
    c[7] = np.nan
    with pytest.raises(CtoError):
        window_dist(c, [0, 20], 100, "host")
    with pytest.raises(CtoError):
        window_dist(np.full(20, 0.4), [0, 12, 8, 20], 100, "host")


@pytest.mark.parametrize("segment_length", [2, 3, 7, 100, 1000])
def test_host_distances_are_numpy_s_bits(segment_length):
    from clairs_to_amd.predict_germline_genotypes import window_dist
    seed = random.SystemRandom().randrange(1 << 30)
    print("seed", seed)
    rng = np.random.default_rng(seed)
    ms = [0, 1, 5, 6, 7, 12, 101, 102, 300, int(rng.integers(6, 250)), 0, int(rng.integers(6, 40))]
    c, off = fresh_runs(rng, ms)
    st = {}
    got = window_dist(c, off, segment_length, "host", st)
    assert st == dict(n_runs=len(ms), n_probes=len(c), host_path=1, kernel_ms=0.0)
    want = np.concatenate([restated_dist(c[a:b], segment_length) for a, b in zip(off[:-1], off[1:])])
    assert same_bits(got, want), (seed, np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0][:5])
    if segment_length >= 5:                                    # m = 6, L = 5: probes 1 and 4 have no defined median
        assert np.isinf(got[off[3] + 1]) and np.isinf(got[off[3] + 4]) and np.isinf(got[off[3]:off[4]]).sum() == 2
    assert (got[off[2]:off[3]] == 1.0).all()


def test_chain_from_count_tables_to_genotypes(tmp_path, monkeypatch):
    """an alleleCounter-format table written here -> get_logr_and_baf --seed -> predict_germline_genotypes: same keys, same order"""
    from clairs_to_amd.__main__ import dispatch
    from clairs_to_amd.allele_counter import HEADER
    monkeypatch.chdir(tmp_path)
    rng = random.Random(5)
    keys = []
    open("contigs.txt", "w").write("chr1\nchr2\n")
    for ctg in ("chr1", "chr2"):
        with open("alleles_%s.txt" % ctg, "w") as fa, open("T_AlleleCount_%s.txt" % ctg, "w") as fc:
            fa.write("position\ta0\ta1\n")
            fc.write(HEADER)
            pos = 0
            for i in range(400):
                pos += rng.randint(100, 3000)
                a0, a1 = rng.sample(range(4), 2)
                counts = [0, 0, 0, 0]
                depth = rng.randint(200, 400)
                alt = sum(rng.random() < (0.5 if i % 3 == 0 else 0.004) for _ in range(depth))
                counts[a0], counts[a1] = depth - alt, alt
                fa.write("%d\t%d\t%d\n" % (pos, a0 + 1, a1 + 1))
                fc.write("%s\t%d\t%d\t%d\t%d\t%d\t%d\n" % (ctg, pos, counts[0], counts[1], counts[2], counts[3], sum(counts)))
                keys.append((ctg, str(pos)))
    dispatch("get_logr_and_baf", ["--tumor_allele_counts_file_prefix", "T_AlleleCount_", "--alleles_file_prefix", "alleles_", "--contig_fn", "contigs.txt",
                                  "--tumor_logr_output_file", "Tumor_LogR.txt", "--tumor_baf_output_file", "Tumor_BAF.txt", "--seed", "11"])
    dispatch("predict_germline_genotypes", ["--tumor_logr_file", "Tumor_LogR.txt", "--tumor_baf_file", "Tumor_BAF.txt",
                                            "--germline_genotypes_output_file", "Tumor_GG.txt", "--where", "host"])
    table = lambda fn: [tuple(r.split("\t")) for r in open(fn).read().split("\n")[1:] if r]
    gg, baf, logr = table("Tumor_GG.txt"), table("Tumor_BAF.txt"), table("Tumor_LogR.txt")
    assert [r[:2] for r in gg] == [r[:2] for r in baf] == [r[:2] for r in logr] == keys
    flags = [r[2] for r in gg]
    assert set(flags) == {"True", "False"}
    assert 0.2 < flags.count("False") / len(flags) < 0.4          # about a third of the loci were written heterozygous
    assert open("Tumor_GG.txt").readline() == "Chromosome\tPosition\tSAMPLE\n"
