"""A plain model of the realigner's fast pass and the windows that test it (tests/test_fast_pass.py, tests/test_gpu_fast_pass.py,
tests/golden/gen_realign.py fastpass).

The model is the ORDER-DEPENDENT definition of the pass, as csrc/realign.cpp (header, Window::fast_pass_host's comments), the fast-pass
section of csrc/realign_batch.hip and DESIGN.md state it: an index of every 32-mer of every read longer than 32; haplotype positions in
ascending order; the occurrences of a position's 32-mer in read order, then offset order; start = max(0, i - o); an occurrence is skipped
when the read does not fit at `start` or its current hit is at `start` already; mismatches counted with N on either side as a match, at
most 2; score 4 * matches - 6 * mismatches, only a strictly larger one replaces a hit; a coverage counter, tested at every position whose
32-mer was found - uncovered, at or after ref_prefix, below the UNSIGNED L - ref_suffix, not the reference: the haplotype is dropped; a
dropped haplotype and one that scores 0 keep no hit.  k_fast_pass computes the same from closed forms (which start wins a tie, since when a
position is covered); `model` returns what both must return, and a trace of the cases a window met, from which every test asserts that
the case it is named for happened.  Test infrastructure only."""
import numpy as np

K = 32
MAX_MISM = 2


def limits():
    from clairs_to_amd.realign_reads import fast_pass_limits
    return fast_pass_limits()


def n_mismatches(hap, start, read):
    return sum(1 for a, b in zip(hap[start:start + len(read)], read) if a != b and a != "N" and b != "N")


def listed_diagonals(hap, read, force0=True):
    """the diagonals d = i - o of one (haplotype, read) pair the kernel lists: a whole 16-aligned block of the read equal on d, plus 0
    (force0: diagonal 0 is listed without such a block, for the mismatch count the clipped diagonals' seeds need)"""
    L, span = len(hap), len(read)
    out = {0} if force0 else set()
    for qb in range(0, span - 15, 16):
        blk, p = read[qb:qb + 16], hap.find(read[qb:qb + 16])
        while p >= 0:
            d = p - qb
            if -(span - K) <= d <= L - K and qb >= max(0, -d):
                out.add(d)
            p = hap.find(blk, p + 1)
    return out


def model(w):
    """(hap_score [H], hit_score [H, n], hit_pos [H, n]) int32 arrays and the trace dict of window w"""
    reads, haps, ref = w["seqs"], w["haplotypes"], w["reference"]
    n, H = len(reads), len(haps)
    index = {}
    for r, s in enumerate(reads):
        if len(s) > K:
            for o in range(len(s) - K + 1):
                index.setdefault(s[o:o + K], []).append((r, o))
    hap_score = np.zeros(H, dtype=np.int32)
    hit_score, hit_pos = np.zeros((H, n), dtype=np.int32), np.full((H, n), -1, dtype=np.int32)
    tr = dict(listed=[], clipped_start0=0, ties=0, dropped=0, dropped_by_time=0, wrapped=0, never_full=0, accepted=0, seeded_rejected=0,
              tie_order_matters=0, kept_scoring=0, start0_forced=0)
    for h, hap in enumerate(haps):
        L = len(hap)
        is_ref = hap == ref
        bound = (L - w["ref_suffix"]) % (1 << 64)                  # the reference computes it in size_t
        tr["wrapped"] += int(w["ref_suffix"] > L)
        cov = [0] * L
        score, pos = [0] * n, [-1] * n
        first_visit = {}                                           # (read, start) -> (i, o) of its first visit, accepted ones
        best_of = {}                                               # read -> {start: first visit} of the starts at its best score
        mism_at = {}
        failed_at = []
        for i in range(L - K + 1):
            occ = index.get(hap[i:i + K])
            if occ is None:
                continue
            for r, o in occ:
                start, span = max(0, i - o), len(reads[r])
                if start + span > L:
                    tr["seeded_rejected"] += 1
                    continue
                if pos[r] == start:
                    continue
                if (r, start) not in mism_at:
                    mism_at[(r, start)] = n_mismatches(hap, start, reads[r])
                mism = mism_at[(r, start)]
                if mism > MAX_MISM:
                    tr["seeded_rejected"] += 1
                    continue
                if (r, start) not in first_visit:
                    first_visit[(r, start)] = (i, o)
                    tr["accepted"] += 1
                    tr["clipped_start0"] += int(start == 0 and i < o)
                    tr["start0_forced"] += int(start == 0 and 0 not in listed_diagonals(hap, reads[r], force0=False))
                sc = 4 * (span - mism) - 6 * mism
                for p in range(start, start + span):
                    cov[p] += 1
                if sc == score[r] and start != pos[r]:
                    tr["ties"] += 1
                    best_of[r][start] = first_visit[(r, start)]
                if sc > score[r]:
                    score[r], pos[r] = sc, start
                    best_of[r] = {start: first_visit[(r, start)]}
            if cov[i] == 0 and i >= w["ref_prefix"] and i < bound and not is_ref:
                failed_at.append(i)                                # (the original stops here; what follows cannot change the result)
        for r, starts in best_of.items():                          # would (o, i) order pick another start than (i, o) order does?
            tr["tie_order_matters"] += int(min(starts, key=lambda s: starts[s]) != min(starts, key=lambda s: starts[s][::-1]))
        dropped = bool(failed_at)
        tr["dropped"] += int(dropped)
        tr["dropped_by_time"] += int(dropped and all(cov[i] > 0 for i in failed_at))
        total = 0 if dropped else sum(score)
        tr["kept_scoring"] += int(total > 0)
        hap_score[h] = total
        if total:
            hit_score[h], hit_pos[h] = score, pos
        tr["listed"].append([len(listed_diagonals(hap, s)) if len(s) > K else 0 for s in reads])
        tr["never_full"] += sum(1 for s in reads if len(s) > L)
    return (hap_score, hit_score, hit_pos), tr


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


def triple_lists(t):
    return [x.tolist() for x in t]


# ---------------------------------------------------------------------------------------------------------------------------------
# windows

def rs(rng, n, alphabet="ACGT"):
    return "".join(alphabet[int(x)] for x in rng.integers(0, len(alphabet), n))


def sub(s, *at):
    """s with the base at every given position replaced by another one (A -> C -> G -> T -> A; N -> A)"""
    b = list(s)
    for p in at:
        b[p] = "CGTAA"["ACGTN".index(b[p])]
    return "".join(b)


def put(s, p, c):
    return s[:p] + c + s[p + len(c):]


def window(reads, starts, reference, haplotypes, prefix=0, suffix=0, ref_start=1000):
    return dict(seqs=list(reads), positions=[ref_start + max(0, int(a)) for a in starts], cigars=["%dM" % len(s) for s in reads],
                reference=reference, haplotypes=list(haplotypes), ref_start=ref_start, ref_prefix=int(prefix), ref_suffix=int(suffix))


def args(w):
    return (w["seqs"], w["positions"], w["cigars"], w["reference"], w["haplotypes"], w["ref_start"], w["ref_prefix"], w["ref_suffix"])


def order_cases():
    """the fixed windows of the rules of order: name -> window"""
    rng = np.random.default_rng(20261021)
    c = {}
    # L = 32: no read longer than 32 fits; one that opens with the haplotype still seeds position 0, which nothing covers
    ref32, hap32 = rs(rng, 32), rs(rng, 32)
    c["L32"] = window([hap32 + "A", hap32], [0, 0], ref32, [ref32, hap32])
    # L = 33: the only start is 0 - exact, one mismatch behind the seed, and a read whose seed lies on diagonal -1
    ref33, hap33 = rs(rng, 33), rs(rng, 33)
    c["L33"] = window([hap33, sub(hap33, 32), "G" + hap33[:32], hap33[:32]], [0, 0, 0, 0], ref33, [hap33, ref33])
    # reads of 32 (not indexed), 33, exactly L (one mismatch), L + 5 (never fits; its seeds count)
    ref = rs(rng, 100)
    hap = sub(ref, 50)
    long_read = hap + rs(rng, 5)
    c["lengths_kept"] = window([hap[10:42], hap[60:93], sub(hap, 40), long_read], [10, 60, 0, 0], ref, [ref, hap], 5, 5)
    c["lengths_dropped"] = window([hap[10:42], long_read, hap[60:93]], [10, 0, 60], ref, [ref, hap], 5, 5)
    # a haplotype that opens with a tandem repeat; reads cut at 0 with one substitution inside their first 32 bases: the 32-mers behind
    # the substitution lie in the repeat and are met at position 0, 1, .. on clipped diagonals before diagonal 0 gets to them
    for unit in (1, 2, 3, 4):
        u = rs(rng, unit)
        while len(set(u)) < min(unit, 2):
            u = rs(rng, unit)
        rep = (u * 60)[:48 + unit]
        tail = rs(rng, 70)
        hap = rep + tail
        ref = sub(hap, 90)
        reads = [sub(hap[:60], 5), sub(hap[:75], 9), hap[:50], sub(hap[unit:unit + 64], 3)]
        c["tandem_start_%d" % unit] = window(reads, [0, 0, 0, unit], ref, [hap, ref], 0, 0)
    # one read, several starts, equal score: the start visited first wins - in (i, o) order, not in (o, i) order
    r = rs(rng, 60)
    hap = rs(rng, 11) + sub(r, 3) + rs(rng, 9) + sub(r, 50) + rs(rng, 13) + sub(r, 20) + rs(rng, 7)      # first visits (15, 4), (80, 0), (174, 21)
    c["tie_two_copies"] = window([r, r[:45], sub(r, 20)], [11, 11, 11], sub(hap, 5), [hap], 0, 0)
    hap = "AC" * 50
    c["tie_tandem"] = window(["AC" * 20, "CA" * 20 + "C", ("AC" * 30)[:55]], [0, 1, 0], "AC" * 30 + "GT" * 20, [hap, "AC" * 30 + "GT" * 20], 0, 0)
    # 2 mismatches are taken, 3 are not
    ref = rs(rng, 100)
    hap = sub(ref, 95)
    c["two_against_three"] = window([sub(hap[10:70], 5, 50), sub(hap[20:80], 5, 10, 15), sub(hap[30:90], 0, 59), sub(hap[5:65], 40, 45, 50)],
                                    [10, 20, 30, 5], ref, [hap, ref], 0, 100)
    # N: a match for the score; a 32-mer with an N is a seed only where the other string holds the N too
    ref = rs(rng, 120)
    hap = sub(ref, 110)
    c["n_in_read"] = window([put(hap[30:70], 20, "N"), put(hap[10:70], 5, "N"), put(sub(hap[40:100], 50, 55), 3, "N")], [30, 10, 40], ref, [hap, ref], 0, 120)
    hapn = put(hap, 50, "N")
    c["n_in_haplotype"] = window([hap[30:70], hap[45:105], sub(hap[20:80], 1, 2)], [30, 45, 20], put(ref, 50, "N"), [hapn, put(ref, 50, "N")], 0, 120)
    c["n_in_both"] = window([hapn[30:70], put(hapn[45:105], 40, "N"), sub(hapn[20:80], 1, 2, 3)], [30, 45, 20], put(ref, 50, "N"), [hapn, put(ref, 50, "N")], 0, 120)
    # the coverage rule: positions 70 .. 78 are seeded by a read that is never accepted
    ref = rs(rng, 120)
    hap = sub(ref, 60)
    cover, offend = hap[:50], sub(hap[70:120], 40, 44, 48)
    c["drop"] = window([cover, offend], [0, 70], ref, [ref, hap], 5, 5)
    c["drop_prefix_beyond"] = window([cover, offend], [0, 70], ref, [ref, hap], 80, 5)
    c["drop_suffix_L"] = window([cover, offend], [0, 70], ref, [ref, hap], 5, 120)
    c["drop_suffix_wraps"] = window([cover, offend], [0, 70], ref, [ref, hap], 5, 170)
    c["drop_suffix_wraps_prefix_beyond"] = window([cover, offend], [0, 70], ref, [ref, hap], 79, 170)
    c["drop_reference"] = window([cover, sub(ref[70:120], 40, 44, 48)], [0, 70], ref, [ref], 5, 5)
    # dropped by the time of the visit alone: position 41 is seeded (by a read that is never accepted) and tested before position 43,
    # where the read that covers it is met first
    ref = rs(rng, 120)
    hap = sub(ref, 110)
    c["drop_by_time"] = window([sub(hap[40:100], 2), sub(hap[41:91], 40, 44, 48)], [40, 41], ref, [hap, ref], 0, 0)
    c["drop_by_time_not"] = window([sub(hap[40:100], 50), sub(hap[41:91], 40, 44, 48)], [40, 41], ref, [hap, ref], 0, 0)
    # the same read twice; no reads; nothing but reads of at most 32 bases
    c["same_read_twice"] = window([hap[20:80], hap[20:80], sub(hap[20:80], 7)], [20, 20, 20], ref, [ref, hap], 10, 10)
    c["no_reads"] = window([], [], ref, [ref, hap], 10, 10)
    c["short_reads_only"] = window([hap[0:32], hap[50:70], hap[88:120], "A"], [0, 50, 88, 0], ref, [ref, hap], 10, 10)
    # a start-0 hit that diagonal 0 alone would never find: both whole 16-blocks of a 40-base read hold a mismatch on diagonal 0, and
    # its only seed is met at position 0 on diagonal -8 (a period-8 haplotype start, broken at 4 and 20)
    u = rs(rng, 4)
    while len(set(u)) < 2:
        u = rs(rng, 4)
    r = [""] * 32 + list(u * 2)
    for q in range(31, -1, -1):
        r[q] = sub(r[q + 8], 0) if q in (4, 20) else r[q + 8]
    r = "".join(r)
    hap = r[8:40] + r[32:40] + rs(rng, 60)
    c["start0_by_clipped_seed_alone"] = window([r], [0], sub(hap, 80), [hap, sub(hap, 80)], 0, 0)
    return c


def random_window(rng, n_hap=None, n_reads=None):
    """a window of the shape of order_cases: L 32 .. 200, two-letter, tandem and plain haplotypes, reads that start up to 10 bases before
    their haplotype and end up to 10 behind it, reads of 32, L and L + 5, prefix and suffix from {0, 5, 30, L, L + 50}"""
    L = int(rng.choice([32, 33, 40, 64, 100, 150, 200])) if rng.random() < 0.4 else int(rng.integers(32, 201))
    style = int(rng.integers(0, 4))
    if style == 0:
        base = rs(rng, L)
    elif style == 1:
        base = rs(rng, L, "AC")
    elif style == 2:
        base = (rs(rng, int(rng.integers(1, 5))) * L)[:int(rng.integers(0, L + 1))]
        base = (base + rs(rng, L))[:L]
    else:
        base = ""
        while len(base) < L:
            base += rs(rng, int(rng.integers(1, 5))) * int(rng.integers(2, 30)) + rs(rng, int(rng.integers(0, 20)))
        base = base[:L]
    H = int(n_hap if n_hap is not None else rng.choice([1, 1, 2, 2, 3, 4]))
    haps = []
    for h in range(H):
        s = base
        if h:
            for _ in range(int(rng.integers(0, 4))):
                s = sub(s, int(rng.integers(0, len(s))))
            if rng.random() < 0.3 and len(s) > 40:
                p = int(rng.integers(0, len(s) - 3))
                s = s[:p] + s[p + int(rng.integers(1, 4)):] if rng.random() < 0.5 else s[:p] + rs(rng, int(rng.integers(1, 4))) + s[p:]
            if rng.random() < 0.1:
                s = put(s, int(rng.integers(0, len(s))), "N")
        haps.append(s)
    ref = haps[int(rng.integers(0, H))] if rng.random() < 0.7 else sub(base, int(rng.integers(0, L)))
    n = int(n_reads if n_reads is not None else rng.integers(1, 9))
    reads, starts = [], []
    for _ in range(n):
        src = haps[int(rng.integers(0, H))]
        Ls = len(src)
        kind = rng.random()
        span = 32 if kind < 0.05 else Ls if kind < 0.15 else Ls + 5 if kind < 0.2 else int(rng.integers(33, 111))
        a = int(rng.integers(-10, max(-9, Ls - span + 11)))
        if rng.random() < 0.3:
            a = 0
        s = "".join(src[p] if 0 <= p < Ls else "ACGT"[int(rng.integers(0, 4))] for p in range(a, a + span))
        for _ in range(int(rng.choice([0, 0, 1, 1, 2, 3]))):
            s = sub(s, int(rng.integers(0, min(span, 32) if rng.random() < 0.5 else span)))
        if rng.random() < 0.08:
            s = put(s, int(rng.integers(0, span)), "N")
        reads.append(s)
        starts.append(a)
    if n_reads is None and rng.random() < 0.15:
        reads.append(reads[0]); starts.append(starts[0])
    L0 = len(haps[0])
    choice = [0, 5, 30, L0, L0 + 50]
    return window(reads, starts, ref, haps, choice[int(rng.integers(0, 5))], choice[int(rng.integers(0, 5))])


def limit_window(rng, L, R):
    """unique random sequence at the kernel's limits: a read on diagonal 0 (exact), one on the last diagonal L - R (one mismatch), in the
    middle one with 3 mismatches and, seven bases before it, one with 2 that covers the seeds of the first"""
    ref = rs(rng, L)
    mid = (L - R) // 2
    hap = sub(ref, R // 2, mid + R // 2, L - R // 2)
    reads = [hap[:R], sub(hap[mid:mid + R], R - 40, R - 30, R - 20), sub(hap[mid - 7:mid - 7 + R], R - 9, R - 5), sub(hap[L - R:], 17)]
    return window(reads, [0, mid, mid - 7, L - R], ref, [ref, hap], 100, 100)


def candidate_window(rng, n_listed):
    """a (haplotype, read) pair with exactly n_listed listed diagonals: the read's only run of A fills its aligned block [16, 32), the
    haplotype holds a run of A of n_listed - 3 + 15 bases (one diagonal per place the block fits), a copy of the read (listed, seeded,
    accepted), the read's last 40 bases behind other sequence (listed, seeded, not accepted) and diagonal 0"""
    lead, tail = rs(rng, 16, "CGT"), rs(rng, 40, "CGT")
    read = lead + "A" * 16 + tail
    hap = (rs(rng, 45, "CGT") + "A" * (n_listed - 3 + 15) + rs(rng, 20, "CGT") + read + rs(rng, 10, "CGT") + rs(rng, 32, "CGT") + tail +
           rs(rng, 25, "CGT"))
    ref = sub(hap, 3)
    at = hap.index(read)
    return window([read, sub(read, 40)], [at, at], ref, [hap, ref], 0, len(hap))


def layout_windows(rng):
    """(H, reads) = (1, 1), (18, 3), (2, 0), (3, 60)"""
    return [random_window(rng, 1, 1), random_window(rng, 18, 3), random_window(rng, 2, 0), random_window(rng, 3, 60)]


LIMIT_SEED, CAND_SEED, LAYOUT_SEED = 20261022, 20261023, 20261024


def limit_cases(lim):
    rng = np.random.default_rng(LIMIT_SEED)
    return {"limit_%dx%d" % (L, R): limit_window(rng, L, R) for L in (lim["FP_LMAX"] - 1, lim["FP_LMAX"]) for R in (lim["FP_RMAX"] - 1, lim["FP_RMAX"])}


def candidate_cases(lim):
    rng = np.random.default_rng(CAND_SEED)
    C = lim["FP_CAND"]
    return {"listed_%d" % n: (n, candidate_window(rng, n)) for n in (C - 1, C, C + 1, 3 * C)}


def layout_cases():
    return layout_windows(np.random.default_rng(LAYOUT_SEED))


def case_windows(lim):
    """every fixed window of the tests, name -> window: what tests/golden/realign_fastpass.json.gz holds the reference's output for"""
    c = dict(order_cases())
    c.update(limit_cases(lim))
    c.update({k: w for k, (_, w) in candidate_cases(lim).items()})
    c.update({"layout_%d" % i: w for i, w in enumerate(layout_cases())})
    return c


# ---------------------------------------------------------------------------------------------------------------------------------
# what the model must have met in each fixed window (the case the window is named for), and - where it follows from the rules by
# hand - what it must return: trace key -> exact value, or (">=", least); "score" / "pos": hit_score / hit_pos rows; "hap": hap_score
EXPECT = {
    "L32": dict(dropped=1, never_full=2, accepted=0, hap=[0, 0]),
    "L33": dict(accepted=2, seeded_rejected=1, score=[[4 * 33, 4 * 32 - 6, 0, 0], [0, 0, 0, 0]], pos=[[0, 0, -1, -1], [-1, -1, -1, -1]]),
    "lengths_kept": dict(never_full=2, dropped=0, score=[[0, 132, 4 * 98 - 12, 0], [0, 132, 4 * 99 - 6, 0]], pos=[[-1, 60, 0, -1]] * 2),
    "lengths_dropped": dict(never_full=2, dropped=1, accepted=2, hap=[132, 0], score=[[0, 0, 132], [0, 0, 0]]),
    "tie_two_copies": dict(ties=(">=", 1), tie_order_matters=1, pos=[[11, 80, 153]], score=[[4 * 59 - 6, 4 * 45, 4 * 60]]),
    "tie_tandem": dict(ties=(">=", 100), pos=[[0, 1, 0]] * 2, score=[[160, 164, 220]] * 2),
    "two_against_three": dict(accepted=4, seeded_rejected=(">=", 2), score=[[4 * 58 - 12, 0, 4 * 58 - 12, 0]] * 2, pos=[[10, -1, 30, -1]] * 2),
    "n_in_read": dict(score=[[0, 240, 4 * 58 - 12]] * 2, pos=[[-1, 10, 40]] * 2),
    "n_in_haplotype": dict(score=[[0, 240, 0]] * 2, pos=[[-1, 45, -1]] * 2),
    "n_in_both": dict(score=[[160, 240, 0]] * 2, pos=[[30, 45, -1]] * 2, seeded_rejected=(">=", 1)),
    "drop": dict(dropped=1, wrapped=0, accepted=2, hap=[200, 0], score=[[200, 0], [0, 0]], pos=[[0, -1], [-1, -1]]),
    "drop_prefix_beyond": dict(dropped=0, wrapped=0, hap=[200, 200]),
    "drop_suffix_L": dict(dropped=0, wrapped=0, hap=[200, 200]),
    "drop_suffix_wraps": dict(dropped=1, wrapped=2, hap=[200, 0]),
    "drop_suffix_wraps_prefix_beyond": dict(dropped=0, wrapped=2, hap=[200, 200]),
    "drop_reference": dict(dropped=0, seeded_rejected=(">=", 1), hap=[200]),
    "drop_by_time": dict(dropped=1, dropped_by_time=1, hap=[0, 230], score=[[0, 0], [230, 0]]),
    "drop_by_time_not": dict(dropped=0, hap=[230, 230]),
    "same_read_twice": dict(accepted=6, score=[[240, 240, 230]] * 2, pos=[[20, 20, 20]] * 2),
    "no_reads": dict(hap=[0, 0], score=[[], []]),
    "short_reads_only": dict(accepted=0, seeded_rejected=0, hap=[0, 0], pos=[[-1] * 4] * 2),
}
EXPECT["start0_by_clipped_seed_alone"] = dict(start0_forced=2, clipped_start0=2, score=[[4 * 38 - 12]] * 2, pos=[[0]] * 2)
EXPECT.update({"tandem_start_%d" % u: dict(clipped_start0=(">=", 3), pos=[[0, 0, 0, u]] * 2, score=[[230, 290, 200, 246]] * 2) for u in (1, 2, 3, 4)})


def check_trace(name, triple, tr, expect=None):
    """the window met the case it is named for (and returns what the rules give by hand)"""
    for key, want in (EXPECT[name] if expect is None else expect).items():
        got = {"hap": triple[0].tolist(), "score": triple[1].tolist(), "pos": triple[2].tolist()}[key] if key in ("hap", "score", "pos") else tr[key]
        if isinstance(want, tuple):
            assert got >= want[1], "%s: the model met %s = %r, the case needs at least %r" % (name, key, got, want[1])
        else:
            assert got == want, "%s: the model has %s = %r, the case needs %r" % (name, key, got, want)


def run(ws, where, **kw):
    from clairs_to_amd.realign_reads import fast_pass_batch
    return fast_pass_batch([args(w) for w in ws], where, **kw)


def assert_equal_to_model(names, ws, got, models, what):
    for name, w, g, m in zip(names, ws, got, models):
        assert same(g, m), "%s: %s has %s, the model %s" % (name, what, triple_lists(g), triple_lists(m))


# ---------------------------------------------------------------------------------------------------------------------------------
# the fixed windows with their models, computed once and shared by the tests of both files (never modified)
_fixed = None


def fixed():
    """name -> (window, model triple, trace) of every fixed window"""
    global _fixed
    if _fixed is None:
        _fixed = {name: (w,) + model(w) for name, w in case_windows(limits()).items()}
    return _fixed


FAMILIES = {
    "lengths": ["L32", "L33", "lengths_kept", "lengths_dropped"],
    "start0": ["tandem_start_1", "tandem_start_2", "tandem_start_3", "tandem_start_4", "start0_by_clipped_seed_alone"],
    "ties": ["tie_two_copies", "tie_tandem"],
    "mismatches_and_n": ["two_against_three", "n_in_read", "n_in_haplotype", "n_in_both"],
    "coverage_rule": ["drop", "drop_prefix_beyond", "drop_suffix_L", "drop_suffix_wraps", "drop_suffix_wraps_prefix_beyond", "drop_reference"],
    "visit_time": ["drop_by_time", "drop_by_time_not"],
    "degenerate": ["same_read_twice", "no_reads", "short_reads_only"],
}


def check_family(family, wheres):
    """every window of the family met its case in the model, and each form in `wheres` returns the model's triple"""
    names = FAMILIES[family]
    ws, ms = [fixed()[k][0] for k in names], [fixed()[k][1] for k in names]
    for k in names:
        check_trace(k, fixed()[k][1], fixed()[k][2])
    for where in wheres:
        assert_equal_to_model(names, ws, run(ws, where), ms, where)                      # in one call
        assert_equal_to_model(names, ws, [run([w], where)[0] for w in ws], ms, where)    # and each alone


def fresh_windows(n=300):
    import os
    seed = int.from_bytes(os.urandom(4), "little")
    print("fresh windows: np.random.default_rng(%d)" % seed)
    rng = np.random.default_rng(seed)
    ws = [random_window(rng) for _ in range(n)]
    return seed, ws, [model(w) for w in ws]


def check_fresh_traces(models):
    """a few hundred windows of this shape meet every case many times over (counts of a typical draw of 300: 86 haplotypes dropped,
    144 wrapped bounds, ~10 000 ties, ~1 000 reads longer than a haplotype) - the least that a draw must hold"""
    tot = {}
    for _, tr in models:
        for k, v in tr.items():
            if k != "listed":
                tot[k] = tot.get(k, 0) + v
    print("fresh windows met:", tot)
    assert tot["dropped"] >= 10 and tot["wrapped"] >= 20 and tot["ties"] >= 100 and tot["never_full"] >= 20 and tot["accepted"] >= 100


def golden_outputs():
    """name -> (positions, cigars) the compiled reference returned on the fixed windows (tests/golden/realign_fastpass.json.gz)"""
    import gzip
    import json
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, "golden"))
    from gen_realign import fastpass_digest
    with gzip.open(os.path.join(here, "golden", "realign_fastpass.json.gz"), "rb") as f:
        g = json.loads(f.read())
    cases = case_windows(limits())
    assert g["limits"] == limits() and fastpass_digest(cases) == g["inputs_sha256"], \
        "the fixed windows changed: regenerate tests/golden/realign_fastpass.json.gz (gen_realign.py fastpass)"
    return {k: ([p + cases[k]["ref_start"] for p, _ in v], [c for _, c in v]) for k, v in g["windows"].items()}
