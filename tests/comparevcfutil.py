"""Test-only: a deliberately naive restatement of compare_vcf's classification (the rules at the top of csrc/comparevcf.hip) - the
reference's four loops over two dicts, with its deletions, and linear scans over the BED intervals; no bisect, no numpy in the rules -
the seeded cases of parallel arrays both compare_vcf test files use, and the reader of tests/golden/compare_vcf.json.gz."""
import functools
import gzip
import json
import os
import random

import numpy as np

HIGHCONF, H, LOWAF = 1, 2, 4
FP, TP, FN, FP_FN, TRUTH, KEPT = 1, 2, 4, 8, 16, 32
COUNTERS = ("tp_snv", "tp_ins", "tp_del", "fp_snv", "fp_ins", "fp_del", "fn_snv", "fn_ins", "fn_del", "gt_mismatch", "input_out_of_bed",
            "truth_out_of_bed", "input_out_of_strat_bed", "truth_out_of_strat_bed", "n_input_left", "n_truth_left")
SIZES = [(0, 0), (1, 0), (0, 1), (1, 1), (63, 65), (64, 64), (65, 63), (257, 1025), (4097, 4095)]


# ------------------------------------------------------------------------------------------ the rules, naively
def holds(case, s, ctg, pos):
    named, off, start, end = case["beds"]
    a, b = off[s * case["n_ctg"] + ctg], off[s * case["n_ctg"] + ctg + 1]
    return any(start[k] <= pos - 1 < end[k] for k in range(a, b))


def naive(case):
    """dict(input_sets, truth_sets, counters, sweep, roc_sweep) as compare_vcf.compare_calls returns it"""
    inp, tru = case["inp"], case["tru"]
    named = [int(x) for x in case["beds"][0]]
    n_sets = len(named)
    bi, hc, skip_gt, vp = case["benchmark_indel"], case["high_confident_only"], case["skip_genotyping"], case["validate_phase"]
    rec = lambda t, i: dict(key=(int(t["ctg"][i]), int(t["pos"][i])), ref_len=int(t["ref_len"][i]), alt_len=int(t["alt_len"][i]), n_alt=int(t["n_alt"][i]),
                            allele=int(t["allele"][i]), gt=[int(t["gt"][i][0]), int(t["gt"][i][1])], flags=int(t["flags"][i]), index=i)
    I = {}
    for i in range(len(inp["pos"])):
        r = rec(inp, i)
        r["qual"] = float(inp["qual"][i])
        I[r["key"]] = r
    T = {}
    for j in range(len(tru["pos"])):
        r = rec(tru, j)
        T[r["key"]] = r
    low_af = set(k for k, r in list(I.items()) + list(T.items()) if r["flags"] & LOWAF)
    for k, r in I.items():                                         # the input half of --validate_phase_only
        phaseable = bool(r["flags"] & H)
        if (vp == 1 and not phaseable) or (vp == 2 and phaseable):
            low_af.add(k)
    low_qual = set(k for k, r in T.items() if hc and not r["flags"] & HIGHCONF)
    in_fp = lambda k: n_sets == 0 or named[0] == 0 or holds(case, 0, k[0], k[1])
    in_strat = lambda k: sum(1 if holds(case, s, k[0], k[1]) else 0 for s in range(1, n_sets)) == max(0, n_sets - 1)
    c = dict.fromkeys(COUNTERS, 0)
    kind = lambda r: "snv" if r["ref_len"] == 1 and r["alt_len"] == 1 else "ins" if r["ref_len"] < r["alt_len"] else "del" if r["ref_len"] > r["alt_len"] else None

    def count(what, r):
        if kind(r):
            c[what + "_" + kind(r)] += 1

    for k in list(I.keys()):
        if not in_fp(k):
            del I[k]
            c["input_out_of_bed"] += 1
            continue
        if not in_strat(k):
            del I[k]
            c["input_out_of_strat_bed"] += 1
            continue
        if hc and k in low_qual:
            continue
        if bi and (kind(I[k]) == "snv" or I[k]["n_alt"] > 1):
            del I[k]
    for k in list(T.keys()):
        if not in_fp(k):
            c["truth_out_of_bed"] += 1
            del T[k]
            continue
        if hc and k in low_qual:
            continue
        if not in_strat(k):
            del T[k]
            c["truth_out_of_strat_bed"] += 1
            continue
        if k in low_af:
            del T[k]
    fp_set, tp_set, fn_set, fp_fn_set, truth_set = set(), set(), set(), set(), set()
    for k, r in I.items():
        if (hc and k in low_qual) or k in low_af:
            continue
        indel = kind(r) in ("ins", "del")
        if k not in T:
            count("fp", r)
            if kind(r) == "snv" or (bi and indel):
                fp_set.add(k)
            continue
        t = T[k]
        gt_match = skip_gt or t["gt"] == r["gt"]
        if not gt_match:
            c["gt_mismatch"] += 1
        if t["allele"] == r["allele"] and gt_match:
            count("tp", r)
            if c["tp_snv"] or kind(t) == "snv":
                tp_set.add(k)
            if bi and indel:
                tp_set.add(k)
        else:
            count("fp", r)
            count("fn", t)
            fp_set.add(k)
            fn_set.add(k)
            if kind(r) == "snv" or kind(t) == "snv" or (bi and kind(t) in ("ins", "del")):
                fp_fn_set.add(k)
        truth_set.add(k)
    truth_fn = set()
    for k, t in T.items():
        if k in truth_set or (hc and k in low_qual) or k in low_af:
            continue
        count("fn", t)
        if kind(t) == "snv" or (bi and kind(t) in ("ins", "del")):
            truth_fn.add(k)
    c["n_input_left"], c["n_truth_left"] = len(I), len(T)
    input_sets, truth_sets = [0] * len(inp["pos"]), [0] * len(tru["pos"])
    for k, r in I.items():
        input_sets[r["index"]] = (KEPT | (FP if k in fp_set else 0) | (TP if k in tp_set else 0) | (FN if k in fn_set else 0) |
                                  (FP_FN if k in fp_fn_set else 0) | (TRUTH if k in truth_set else 0))
    for k, t in T.items():
        truth_sets[t["index"]] = KEPT | (FN if k in truth_fn else 0)
    quals = [float(q) for q in inp["qual"]]
    sweep = lambda cuts: np.array([[sum(1 for q, s in zip(quals, input_sets) if s & bit and q >= cut) for bit in (FP, TP)] for cut in cuts],
                                  dtype=np.int64).reshape(len(cuts), 2)
    return dict(input_sets=np.array(input_sets, dtype=np.uint8), truth_sets=np.array(truth_sets, dtype=np.uint8), counters=c,
                sweep=sweep([float(x) for x in case["cutoffs"]]), roc_sweep=sweep([float(x) for x in case["roc_cutoffs"]]))


def naive_sweep(values, sets, cutoffs):
    return np.array([[sum(1 for v, s in zip(values, sets) if s & bit and v >= c) for bit in (FP, TP)] for c in cutoffs], dtype=np.int64).reshape(len(cutoffs), 2)


# ------------------------------------------------------------------------------------------ seeded cases
N_CTG = 4                                                          # contig 3 never has an interval


def _table(rng, n, span, with_qual):
    keys = rng.sample([(c, p) for c in range(N_CTG) for p in range(1, span + 1)], n)
    lens = [(1, 1), (1, 1), (1, 1), (1, 2), (1, 4), (3, 1), (2, 1), (2, 2)]
    t = dict(ctg=np.array([k[0] for k in keys], dtype=np.int32).reshape(n), pos=np.array([k[1] for k in keys], dtype=np.int32).reshape(n),
             n_alt=np.array([rng.choice((1, 1, 1, 2)) for _ in range(n)], dtype=np.int32).reshape(n),
             gt=np.array([rng.choice(((0, 1), (0, 1), (1, 1), (0, 0), (-1, -1))) for _ in range(n)], dtype=np.int32).reshape(n, 2),
             flags=np.array([rng.choice((0, 1, 1, 1, 2, 3, 3, 5, 4)) for _ in range(n)], dtype=np.uint8).reshape(n))
    rl = [rng.choice(lens) for _ in range(n)]
    t["ref_len"], t["alt_len"] = np.array([x[0] for x in rl], dtype=np.int32).reshape(n), np.array([x[1] for x in rl], dtype=np.int32).reshape(n)
    # the allele id is a function of the lengths and one of two spellings: equal ids -> equal lengths, as for strings
    t["allele"] = np.array([(a * 8 + b) * 2 + rng.choice((0, 0, 0, 1)) for a, b in rl], dtype=np.int32).reshape(n)
    if with_qual:
        t["qual"] = np.array([rng.choice((float("nan"), -1.5, -0.0, 0.0, 0.5, 3.0, 3.0, 3.25, 17.0, rng.randrange(0, 400) / 8.0)) for _ in range(n)],
                             dtype=np.float64).reshape(n)
    return t


def _beds(rng, n_sets, span, inp, tru, last_names_none):
    """sorted, merged intervals per (set, contig).  Set 0 names no contig in one case out of four; the last of three sets names none when the seed is odd; contig 3
    has no interval anywhere, contig 2 one interval per set; around a few records' positions the four boundary cases are planted."""
    named, off, start, end = [], [0], [], []
    pts = [int(p) for p in list(inp["pos"][:6]) + list(tru["pos"][:6])]
    for s in range(n_sets):
        empty = (s == 0 and rng.random() < 0.25) or (s == 2 and last_names_none)
        n_named = 0
        for c in range(N_CTG):
            ivs = []
            if not empty and c < 3:
                if c == 2:
                    ivs = [(span // 4, span)]
                else:
                    raw = [(a, a + rng.randrange(1, max(2, span // 6))) for a in (rng.randrange(0, span + 2) for _ in range(rng.randrange(1, 9)))]
                    for p in pts:                                 # pos - 1 == start, == end - 1, == end; pos == start
                        raw.append(rng.choice(((p - 1, p + 2), (max(0, p - 3), p), (max(0, p - 4), p - 1), (p, p + 1))))
                    for a, b in sorted((a, b) for a, b in raw if a >= 0 and b > a):
                        if ivs and a <= ivs[-1][1]:
                            ivs[-1] = (ivs[-1][0], max(ivs[-1][1], b))
                        else:
                            ivs.append((a, b))
            n_named += bool(ivs)
            start += [a for a, _ in ivs]
            end += [b for _, b in ivs]
            off.append(len(start))
        named.append(n_named)
    return (np.array(named, dtype=np.int32), np.array(off if n_sets else [0], dtype=np.int64), np.array(start, dtype=np.int64),
            np.array(end, dtype=np.int64))


@functools.lru_cache(maxsize=None)
def seeded_case(n_in, n_tr, n_sets, seed=0):
    """one case of parallel arrays; switches and the validate_phase gate follow from the seed"""
    rng = random.Random(1000003 * seed + 7919 * n_in + 31 * n_tr + n_sets)
    span = max(8, (n_in + n_tr) // 3)                              # dense enough that a good share of the keys is on both sides
    inp, tru = _table(rng, n_in, span, True), _table(rng, n_tr, span, False)
    # a share of the common keys agrees in allele and genotype
    at = {(int(c), int(p)): j for j, (c, p) in enumerate(zip(tru["ctg"], tru["pos"]))}
    for i, k in enumerate(zip(inp["ctg"].tolist(), inp["pos"].tolist())):
        j = at.get(k)
        if j is not None and rng.random() < 0.6:
            for col in ("ref_len", "alt_len", "allele"):
                inp[col][i] = tru[col][j]
            if rng.random() < 0.7:
                inp["gt"][i] = tru["gt"][j]
    finite = inp["qual"][np.isfinite(inp["qual"])]
    case = dict(inp=inp, tru=tru, beds=_beds(rng, n_sets, span, inp, tru, n_sets == 3 and seed % 2 == 1), n_ctg=N_CTG, benchmark_indel=rng.random() < 0.5,
                high_confident_only=rng.random() < 0.5, skip_genotyping=rng.random() < 0.5, validate_phase=rng.choice((0, 0, 1, 2)),
                cutoffs=np.unique(np.trunc(finite)), roc_cutoffs=np.unique(finite))
    for t in (inp, tru):
        for a in t.values():
            a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def seeded_expected(n_in, n_tr, n_sets, seed=0):
    """naive() of a seeded case: computed once, shared by every test that needs it (read-only)"""
    return naive(seeded_case(n_in, n_tr, n_sets, seed))


def running_count_case(n, snv_at):
    """rule 10 alone: n insertion calls that equal their truth records, without --benchmark_indel; record `snv_at` (None: none) is an SNV
    that equals its truth record.  tp_set is every record from snv_at on."""
    is_snv = np.arange(n) == (-1 if snv_at is None else snv_at)
    one = lambda v: np.full(n, v, dtype=np.int32)
    t = dict(ctg=one(0), pos=np.arange(1, n + 1, dtype=np.int32), ref_len=one(1), alt_len=np.where(is_snv, 1, 2).astype(np.int32), n_alt=one(1),
             allele=np.where(is_snv, 1, 2).astype(np.int32), gt=np.tile(np.array([[0, 1]], dtype=np.int32), (n, 1)), flags=np.zeros(n, dtype=np.uint8))
    none = (np.zeros(0, dtype=np.int32), np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
    return dict(inp=dict(t, qual=np.arange(n, dtype=np.float64)), tru=dict(t), beds=none, n_ctg=1, benchmark_indel=False, high_confident_only=False,
                skip_genotyping=True, validate_phase=0, cutoffs=np.zeros(0), roc_cutoffs=np.zeros(0))


def run_case(case, where, host_threads=0):
    from clairs_to_amd.compare_vcf import compare_calls
    return compare_calls(case["inp"], case["tru"], case["beds"], case["n_ctg"], case["benchmark_indel"], case["high_confident_only"],
                         case["skip_genotyping"], case["validate_phase"], case["cutoffs"], case["roc_cutoffs"], where=where, host_threads=host_threads)


def assert_same(got, want):
    for k in ("input_sets", "truth_sets", "sweep", "roc_sweep"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert got["counters"] == want["counters"]


def sweep_values(n, n_cut, seed=0):
    """(values, sets, cutoffs) of the sweep tests: values equal to a cut-off, NaN values, negative values against the cut-off 0"""
    rng = random.Random(97 * n + n_cut + seed)
    cutoffs = [0.0] + [rng.choice((-2.0, 0.5, 1.0, 7.0, 7.25, 30.0, rng.randrange(-40, 400) / 4.0)) for _ in range(n_cut - 1)]
    values = [rng.choice((float("nan"), -1.0, -0.25, -0.0, 0.0, rng.choice(cutoffs), rng.choice(cutoffs) + 0.125, rng.randrange(-40, 400) / 4.0)) for _ in range(n)]
    sets = [rng.choice((0, FP, TP, FP | TP, FP | FN | KEPT)) for _ in range(n)]
    return np.array(values, dtype=np.float64), np.array(sets, dtype=np.uint8), np.array(cutoffs, dtype=np.float64)


# ------------------------------------------------------------------------------------------ the fixture
@functools.lru_cache(maxsize=None)
def golden():
    """tests/golden/compare_vcf.json.gz (gen_compare_vcf.py: the reference's compare_vcf on the texts it stores)"""
    return json.load(gzip.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "compare_vcf.json.gz"), "rt"))


def write_inputs(d):
    """the fixture's input texts into directory d, under the names its configurations use; `.gz` names are gzip-compressed"""
    for name, text in golden()["inputs"].items():
        with (gzip.open(os.path.join(d, name), "wt") if name.endswith(".gz") else open(os.path.join(d, name), "w")) as f:
            f.write(text)


def config_argv(cf, d, out, where, bam=None):
    """the command line of one fixture configuration: its stored argv with the input files in d and the outputs in `out`"""
    argv = [a.replace("@IN@", str(d)).replace("@OUT@", str(out)).replace("@BAM@", str(bam)).replace("@SAMTOOLS@", "samtools") for a in cf["argv"]]
    return argv + ["--where", where]
