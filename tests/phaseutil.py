"""Test-only: the phasing rules of csrc/phase.hip restated naively over bamutil read dicts, a read set built by hand with what the
rules make of it written out, and the tests/golden/hapsim.py simulations as phasing cases with their truth."""
import bisect
import os
import sys

import bamutil

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, "golden") not in sys.path:
    sys.path.insert(0, os.path.join(HERE, "golden"))


# ------------------------------------------------------------------------------------------ the rules, naively
def entered(reads, ref_index, sites, min_mq=20, excl_flags=2316):
    """indices of the reads that enter: cto_af_tallies' acceptance over pos[0] .. pos[n - 1]"""
    lo, hi = sites[0][0] - 1, sites[-1][0]              # 0-based [lo, hi)
    out = []
    for i, r in enumerate(reads):
        if r["ref"] != ref_index or (r["flag"] & excl_flags) or (r["flag"] & 4) or r["mapq"] < min_mq:
            continue
        if (r["flag"] & 1) and not (r["flag"] & 2):
            continue
        cigar = bamutil.effective_cigar(r)
        if not cigar or not r["seq"] or r["pos"] < 0 or sum(n for op, n in cigar if op in bamutil.CONSUMES_QUERY) != len(r["seq"]):
            continue
        rl = bamutil.ref_len_of(cigar)
        if rl == 0 or r["pos"] >= hi or r["pos"] + rl <= lo:
            continue
        out.append(i)
    return out


def observations(read, sites):
    """[(site index, allele)] of one read, ascending: rule a"""
    at = {}
    rp, qp = read["pos"], 0
    for op, n in bamutil.effective_cigar(read):
        if op in "M=X":
            for k in range(n):
                at[rp + k] = read["seq"][qp + k]
        if op in bamutil.CONSUMES_REF:
            rp += n
        if op in bamutil.CONSUMES_QUERY:
            qp += n
    out = []
    for s, (pos, ref, alt) in enumerate(sites):
        b = at.get(pos - 1)
        if b is None or b not in "ACGT":
            continue
        if b == ref.upper():
            out.append((s, 0))
        elif b == alt.upper():
            out.append((s, 1))
    return out


def link_table(obs, n, K):
    """rule b -> {(a, b - a - 1, differ): count}, zeros left out"""
    link = {}
    for o in obs:
        for i, (a, x) in enumerate(o):
            for b, y in o[i + 1:]:
                if b - a <= K:
                    key = (a, b - a - 1, int(x != y))
                    link[key] = link.get(key, 0) + 1
    return link


def phase_pass(link, sites, K):
    """rule c -> (phase, ps, block) per site"""
    n = len(sites)
    phase, ps, block = [-1] * n, [0] * n, [-1] * n
    cur = -1
    for b in range(n):
        same = flip = 0
        for a in range(max(0, b - K), b):
            if block[a] != cur or cur < 0:
                continue
            eq, ne = link.get((a, b - a - 1, 0), 0), link.get((a, b - a - 1, 1), 0)
            same += eq if phase[a] == 0 else ne
            flip += ne if phase[a] == 0 else eq
        T = same + flip
        if b == 0 or T < 2:
            cur += 1
            phase[b], block[b], ps[b] = 0, cur, sites[b][0]
        elif 4 * min(same, flip) > T:
            continue
        else:
            phase[b], block[b] = int(flip > same), cur
            ps[b] = next(sites[a][0] for a in range(n) if block[a] == cur)
    return phase, ps, block


def assign(obs, phase, ps, block):
    """rule d -> [(HP, PS)] per read"""
    out = []
    for o in obs:
        votes = {}
        for s, x in o:
            if phase[s] >= 0:
                votes.setdefault(block[s], [0, 0])[x ^ phase[s]] += 1
        best = None
        for blk in sorted(votes):
            if best is None or sum(votes[blk]) > sum(votes[best]):
                best = blk
        hp, p = 0, 0
        if best is not None:
            h1, h2 = votes[best]
            hp = 1 if 10 * h1 >= 6 * (h1 + h2) else (2 if 10 * h2 >= 6 * (h1 + h2) else 0)
            p = next(ps[s] for s in range(len(ps)) if block[s] == best) if hp else 0
        out.append((hp, p))
    return out


def naive(reads, ref_index, sites, K=8, min_mq=20, excl_flags=2316):
    """the whole of it -> dict(entered (indices into reads), obs, link (dict), phase, ps, tags [(HP, PS)])"""
    ent = entered(reads, ref_index, sites, min_mq, excl_flags)
    obs = [observations(reads[i], sites) for i in ent]
    link = link_table(obs, len(sites), K)
    phase, ps, block = phase_pass(link, sites, K)
    return dict(entered=ent, obs=obs, link=link, phase=phase, ps=ps, tags=assign(obs, phase, ps, block))


# ------------------------------------------------------------------------------------------ the library's result in the same shape
def voffs_of(info):
    """the virtual offset of every record of a bamutil.write_bam file, from what write_bam returned"""
    ustarts = [0]
    for s in info["block_sizes"][:-1]:
        ustarts.append(ustarts[-1] + s)
    out = []
    for u, _ in info["record_spans"]:
        k = bisect.bisect_right(ustarts, u) - 1
        out.append((info["block_offsets"][k] << 16) | (u - ustarts[k]))
    return out


def shaped(res, K):
    """phase_tumor.phase_reads' dict as naive() gives it, the reads named by their virtual offsets"""
    obs = [[(int(o) >> 1, int(o) & 1) for o in res["obs"][res["obs_off"][r]:res["obs_off"][r + 1]]] for r in range(len(res["voff"]))]
    link = {}
    for a in range(res["link"].shape[0]):
        for d in range(K):
            for x in (0, 1):
                if res["link"][a, d, x]:
                    link[(a, d, x)] = int(res["link"][a, d, x])
    return dict(voff=[int(v) for v in res["voff"]], obs=obs, link=link, phase=[int(x) for x in res["phase"]], ps=[int(x) for x in res["ps"]],
                tags=[(int(h), int(p)) for h, p in zip(res["hp"], res["read_ps"])])


def assert_same_arrays(a, b):
    """two phase_reads results, array for array"""
    import numpy as np
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------ a read set built by hand
HAND_CTG, HAND_LEN = "p1", 3000
# eight sites, REF A and ALT C at each (lower case at two: the letters are upper-cased); haplotype 1 carries 0 1 0 . 1 0 | 0 1
HAND_SITES = [(100, "A", "C"), (200, "a", "C"), (300, "A", "c"), (400, "A", "C"), (500, "A", "C"), (600, "A", "C"), (2000, "A", "C"), (2100, "A", "C")]
HAND_BLOCK_PAYLOAD = 97


def hand_reads():
    """Twenty reads, seventeen of which enter.  Reference and reads are all A except where a read says otherwise."""
    def rd(name, start, end, bases, flag=0, mapq=60, cigar=None, **kw):
        cigar = cigar or [("M", end - start)]
        qlen = sum(n for op, n in cigar if op in bamutil.CONSUMES_QUERY)
        seq = ["A"] * qlen
        # the query index of a reference position, through the CIGAR
        rp, qp, qi = start, 0, {}
        for op, n in cigar:
            if op in "M=X":
                for k in range(n):
                    qi[rp + k] = qp + k
            if op in bamutil.CONSUMES_REF:
                rp += n
            if op in bamutil.CONSUMES_QUERY:
                qp += n
        for pos1, b in bases.items():
            if pos1 - 1 in qi:                          # a deleted or skipped position has no base to set
                seq[qi[pos1 - 1]] = b
        return dict(name=name, flag=flag, ref=0, pos=start, mapq=mapq, cigar=cigar, seq="".join(seq), qual=[30] * qlen, **kw)
    h1 = {100: "A", 200: "C", 300: "A", 500: "C", 600: "A", 2000: "A", 2100: "C"}
    h2 = {100: "C", 200: "A", 300: "C", 500: "A", 600: "C", 2000: "C", 2100: "A"}
    pick = lambda h, lo, hi: {p: b for p, b in h.items() if lo < p <= hi}
    reads = [
        rd("A1", 50, 350, pick(h1, 50, 350)),
        rd("A2", 50, 350, pick(h2, 50, 350), flag=16),                                   # reverse strand
        rd("A3", 50, 650, pick(h1, 50, 650) | {400: "C"}),                               # site 400: ALT on both haplotypes ...
        rd("A4", 50, 650, pick(h2, 50, 650) | {400: "C"}),
        rd("D1", 50, 350, pick(h1, 50, 350), cigar=[("M", 149), ("D", 1), ("M", 150)]),  # a deletion over site 200
        rd("N1", 50, 350, pick(h2, 50, 350), cigar=[("M", 149), ("N", 1), ("M", 150)]),  # a reference skip over site 200
        rd("T1", 50, 350, pick(h1, 50, 350) | {200: "G"}),                               # a third allele at site 200
        rd("I1", 50, 350, pick(h2, 50, 350), cigar=[("M", 150), ("I", 2), ("M", 150)]),  # an insertion directly behind site 200's base
        rd("X1", 50, 250, {100: "A", 200: "A"}),                                         # one vote each way: h1 = h2
        rd("Q1", 50, 650, {p: "C" for p in (100, 200, 300, 400, 500, 600)}, mapq=19),    # MAPQ below min_mq
        rd("F1", 50, 650, {p: "C" for p in (100, 200, 300, 400, 500, 600)}, flag=256),   # an excluded flag
        rd("O1", 50, 650, {p: "C" for p in (100, 200, 300, 400, 500, 600)}, flag=1),     # an orphan
        rd("V1", 50, 650, {100: "A", 200: "C", 300: "A", 400: "G", 500: "A", 600: "C"}),  # three votes of five for haplotype 1
        rd("A5", 150, 650, pick(h1, 150, 650)),                                          # ... and REF on both
        rd("A6", 150, 650, pick(h2, 150, 650)),
        rd("S1", 550, 2150, pick(h1, 550, 2150)),                                        # the one read over the stretch: both blocks
        rd("Z1", 700, 800, {}),                                                          # covers no site
        rd("B1", 1950, 2150, pick(h1, 1950, 2150)),
        rd("B2", 1950, 2150, pick(h2, 1950, 2150)),
        rd("B3", 1950, 2150, pick(h1, 1950, 2150)),
    ]
    assert [r["pos"] for r in reads] == sorted(r["pos"] for r in reads)
    return reads


# What the rules make of them, written out by hand.  Observations as {read: [(site, allele)]}, in file order.
HAND_OBS = [
    ("A1", [(0, 0), (1, 1), (2, 0)]), ("A2", [(0, 1), (1, 0), (2, 1)]),
    ("A3", [(0, 0), (1, 1), (2, 0), (3, 1), (4, 1), (5, 0)]), ("A4", [(0, 1), (1, 0), (2, 1), (3, 1), (4, 0), (5, 1)]),
    ("D1", [(0, 0), (2, 0)]), ("N1", [(0, 1), (2, 1)]), ("T1", [(0, 0), (2, 0)]), ("I1", [(0, 1), (1, 0), (2, 1)]),
    ("X1", [(0, 0), (1, 0)]), ("V1", [(0, 0), (1, 1), (2, 0), (4, 0), (5, 1)]),
    ("A5", [(1, 1), (2, 0), (3, 0), (4, 1), (5, 0)]), ("A6", [(1, 0), (2, 1), (3, 0), (4, 0), (5, 1)]),
    ("S1", [(5, 0), (6, 0), (7, 1)]), ("Z1", []), ("B1", [(6, 0), (7, 1)]), ("B2", [(6, 1), (7, 0)]), ("B3", [(6, 0), (7, 1)]),
]
# link[a][b - a - 1][differ] at K = 8, zeros left out
HAND_LINK = {
    (0, 0, 0): 1, (0, 0, 1): 6,                                     # 100-200: X1 alone has equal alleles
    (0, 1, 0): 9,                                                    # 100-300: A1 A2 A3 A4 D1 N1 T1 I1 V1, all equal
    (0, 2, 0): 1, (0, 2, 1): 1,                                      # 100-400: A4 equal, A3 differ
    (0, 3, 0): 1, (0, 3, 1): 2,                                      # 100-500: V1 equal; A3 A4 differ
    (0, 4, 0): 2, (0, 4, 1): 1,                                      # 100-600: A3 A4 equal; V1 differ
    (1, 0, 1): 8,                                                    # 200-300: A1 A2 A3 A4 I1 V1 A5 A6
    (1, 1, 0): 2, (1, 1, 1): 2,                                      # 200-400: A3 A6 equal; A4 A5 differ
    (1, 2, 0): 4, (1, 2, 1): 1,                                      # 200-500: A3 A4 A5 A6 equal; V1 differ
    (1, 3, 0): 1, (1, 3, 1): 4,                                      # 200-600
    (2, 0, 0): 2, (2, 0, 1): 2,                                      # 300-400: A4 A5 equal; A3 A6 differ - the tie
    (2, 1, 0): 1, (2, 1, 1): 4,                                      # 300-500
    (2, 2, 0): 4, (2, 2, 1): 1,                                      # 300-600
    (3, 0, 0): 2, (3, 0, 1): 2,                                      # 400-500
    (3, 1, 0): 2, (3, 1, 1): 2,                                      # 400-600
    (4, 0, 1): 5,                                                    # 500-600: A3 A4 V1 A5 A6
    (5, 0, 0): 1, (5, 1, 1): 1,                                      # 600-2000, 600-2100: S1 alone
    (6, 0, 1): 4,                                                    # 2000-2100: S1 B1 B2 B3
}
HAND_PHASE = [0, 1, 0, -1, 1, 0, 0, 1]                               # site 400: same = flip = 5 of 10
HAND_PS = [100, 100, 100, 0, 100, 100, 2000, 2000]
HAND_TAGS = {"A1": (1, 100), "A2": (2, 100), "A3": (1, 100), "A4": (2, 100), "D1": (1, 100), "N1": (2, 100), "T1": (1, 100), "I1": (2, 100),
             "X1": (0, 0),                                           # h1 = h2 = 1
             "V1": (1, 100),                                         # 3 of 5: 30 >= 30
             "A5": (1, 100), "A6": (2, 100),
             "S1": (1, 2000),                                        # one vote in the first block, two in the second
             "Z1": (0, 0), "B1": (1, 2000), "B2": (2, 2000), "B3": (1, 2000)}


def write_hand_bam(path, level=6):
    reads = hand_reads()
    info = bamutil.write_bam(str(path), [(HAND_CTG, HAND_LEN)], reads, block_payload=HAND_BLOCK_PAYLOAD, level=level)
    return reads, info


# ------------------------------------------------------------------------------------------ simulated truth
SIM_CTG = "chr1"
SIM_SEEDS = (7, 11, 23)


def sim_case(seed):
    """hapsim.simulate(seed) as a phasing case: dict(reads (bamutil dicts), ref_len, sites [(pos, REF, ALT)] - the germline 0/1 SNPs and
    the SNV calls, as a tumour-only VCF holds them -, germline {site index: the haplotype that carries ALT}, hap [truth haplotype per read])"""
    import hapsim
    import haputil
    sim = hapsim.simulate(seed)
    reads = haputil.reads_of(sim)
    germ = {g[0]: (g[1], g[2]) for g in sim["germline"] if g[3] == "0/1" and len(g[1]) == 1 and len(g[2]) == 1}
    at = dict(germ)
    for pos, ref, alt in sim["snv_calls"]:
        at.setdefault(pos, (ref, alt))
    sites = [(p, at[p][0], at[p][1]) for p in sorted(at)]
    carrier = {}
    for s, (pos, ref, alt) in enumerate(sites):
        if pos not in germ:
            continue
        n = [0, 0, 0]
        for r in sim["reads"]:
            if r["edits"].get(pos - 1) == ("X", alt):
                n[r["hap"]] += 1
        carrier[s] = 1 if n[1] > n[2] else 2
    return dict(reads=reads, ref_len=len(sim["ref"]), sites=sites, germline=carrier, hap=[r["hap"] for r in sim["reads"]],
                n_calls=len(sites) - len(carrier))


def write_sim_bam(path, case, level=6, block_payload=3000):
    return bamutil.write_bam(str(path), [(SIM_CTG, case["ref_len"])], case["reads"], block_payload=block_payload, level=level)


def quality(case, got, entered_idx):
    """got: shaped() or naive() output whose reads are case['reads'][entered_idx[k]] -> dict(switch_errors, phased, n_germline, eligible,
    tagged_eligible, tagged, wrong)"""
    phase, ps = got["phase"], got["ps"]
    germ = sorted(case["germline"])
    # a block's label: does its haplotype 1 carry the simulation's haplotype 1?  x = 0 when it does.
    x_of = {s: phase[s] ^ (1 if case["germline"][s] == 1 else 0) for s in germ if phase[s] >= 0}
    switch, label, last = 0, {}, {}
    for s in germ:
        if phase[s] < 0:
            continue
        if ps[s] in last and last[ps[s]] != x_of[s]:
            switch += 1
        last[ps[s]] = x_of[s]
        label.setdefault(ps[s], []).append(x_of[s])
    swap = {p: int(2 * sum(v) > len(v)) for p, v in label.items()}
    eligible = tagged_eligible = tagged = wrong = 0
    for k, i in enumerate(entered_idx):
        n_germ = sum(1 for s, _ in got["obs"][k] if s in case["germline"])
        hp, p = got["tags"][k]
        if n_germ >= 2:
            eligible += 1
            tagged_eligible += hp != 0
        if hp:
            tagged += 1
            truth = case["hap"][i]
            mine = hp if not swap.get(p, 0) else 3 - hp
            wrong += mine != truth
    return dict(switch_errors=switch, phased=sum(1 for s in germ if phase[s] >= 0), n_germline=len(germ), eligible=eligible,
                tagged_eligible=tagged_eligible, tagged=tagged, wrong=wrong,
                calls_unphased=sum(1 for s in range(len(phase)) if s not in case["germline"] and phase[s] < 0))
