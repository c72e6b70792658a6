"""Builders of the pile-up shape tests (tests/test_pileup_shapes.py: the host reader against the naive pile-up; tests/
test_gpu_pileup_shapes.py: csrc/pileup.hip against the host reader): long reads of hundreds to tens of thousands of CIGAR operations
and the limits pileup.hip sets for itself - 2048 reads in a column, 2047 open at a read's start, 64 indel keys in a column.
Every builder is a plain function of a fixed seed: a failing case is the same case on the next run.  Each returns a Case:
refs [(name, length)], ref_seqs, reads (dicts as bamutil.write_bam takes them: unpaired, without N operations, sorted by position),
regions [(contig index, start, end, bed or None, max_depth)] (1-based inclusive, BED 0-based half-open) and figs, the figures the
tests assert on so that a case is the case it claims to be (assert_reach)."""
import collections
import functools

import numpy as np

from bamutil import CONSUMES_QUERY, mpileup_rows, ref_len_of, write_bam

Case = collections.namedtuple("Case", "refs ref_seqs reads regions figs")

ALIGNED = "M=X"
EXCL_FLAGS = 2316
PLANTED_RUNS = (47, 48, 49, 63, 64, 65, 255, 256, 257)      # around LONG_OP = 48, one 64-position slice, one 256-position trip
ARRAYS = ("col_pos", "col_ref", "col_off", "key_off", "entries", "key_meta", "key_group")


def _bases(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(list(alphabet), size=n)) if n else ""


def _read(rng, name, flag, ref, pos, cigar, mapq=60, alphabet="ACGT", no_qual=False, cg_tag=False, seq=None):
    qlen = sum(n for op, n in cigar if op in CONSUMES_QUERY)
    if seq is None:
        seq = _bases(rng, qlen, alphabet)
    assert len(seq) == qlen and pos >= 0
    qual = None if no_qual else [int(q) for q in rng.integers(0, 100, size=qlen)]
    return dict(name=name, flag=int(flag), ref=ref, pos=int(pos), mapq=int(mapq), cigar=list(cigar), seq=seq, qual=qual, cg_tag=bool(cg_tag))


def accepted(read, ref, min_mq=0):
    """the header filters of the pile-up (--excl-flags 2316, unmapped, MAPQ), restated"""
    return read["ref"] == ref and not (read["flag"] & (EXCL_FLAGS | 4)) and read["mapq"] >= min_mq


def open_at_starts(reads, ref, min_mq=0):
    """per accepted read, in file order: the number of earlier accepted reads that end behind its start"""
    acc = [r for r in reads if accepted(r, ref, min_mq)]
    pos = np.array([r["pos"] for r in acc], dtype=np.int64)
    end = np.array([r["pos"] + ref_len_of(r["cigar"]) for r in acc], dtype=np.int64)
    return [int((end[:j] > pos[j]).sum()) for j in range(len(acc))]


def aligned_runs(read):
    """(0-based start, length) of every M / = / X operation"""
    out, rp = [], read["pos"]
    for op, n in read["cigar"]:
        if op in ALIGNED:
            out.append((rp, n))
        if op in "MDN=X":
            rp += n
    return out


def cigar_figures(reads, ref):
    acc = [r for r in reads if accepted(r, ref)]
    runs = [n for r in acc for _, n in aligned_runs(r)]
    return dict(max_ops=max(len(r["cigar"]) for r in acc), min_ops=min(len(r["cigar"]) for r in acc),
                n_over_64=sum(len(r["cigar"]) > 64 for r in acc), longest_run=max(runs), run_lengths=set(runs),
                n_p_at_boundary=sum(any(len(r["cigar"]) > b and r["cigar"][b][0] == "P" and r["cigar"][b - 1][0] in ALIGNED for b in (64, 128))
                                    for r in acc),
                n_cg=sum(r["cg_tag"] for r in acc), max_open=max(open_at_starts(reads, ref)))


def _separator(rng):
    n = int(rng.integers(61, 71)) if rng.random() < 0.02 else int(rng.integers(1, 6))     # a few over max_indel_length
    u = rng.random()
    if u < 0.45:
        return [("I", n)]
    if u < 0.90:
        return [("D", n)]
    if u < 0.94:
        return [("D", n), ("I", 1)]                  # an insertion right behind a deletion: attached to nothing
    if u < 0.97:
        return [("P", 1), ("I", n)]
    return []                                        # the next aligned run follows directly (M then X, say)


def _long_cigar(rng, n_runs, span, plant_runs=(), plant_at=None, lead=()):
    """`lead`, then n_runs aligned runs of 1.. bases (plant_runs among them) with short indels between them, about `span` reference
    bases in all.  plant_at = {operation index b: operations}: operation b - 1 is made an aligned run and the operations are put
    behind it at index b, in front of the next aligned run - the look-ahead of the run's last base then starts at index b."""
    n_short = n_runs - len(plant_runs)
    mean = max(2, (span - sum(plant_runs) - 2 * n_runs) // n_short)
    runs = [int(x) for x in rng.integers(1, 2 * mean, size=n_short)]
    for L in plant_runs:
        runs.insert(int(rng.integers(0, len(runs) + 1)), int(L))
    ops = list(lead)
    for L in runs:
        ops.append((str(rng.choice(list("MMMM=X"))), L))
        ops += _separator(rng)
    while ops[-1][0] not in ALIGNED:
        ops.pop()
    for b in sorted(plant_at or {}):
        if ops[b - 1][0] not in ALIGNED:
            ops.insert(b - 1, ("X", 2))
        while ops[b][0] not in ALIGNED:
            del ops[b]
        ops[b:b] = plant_at[b]
    return ops


def _windows(lo, hi, width, step):
    return [(a, a + width) for a in range(lo, hi - width, step)]


LONG_REGIONS = ("whole", "bed33", "bed1", "run_edges", "cut")


def long_reads(seed=101, n_reads=120, L=20000):
    """long reads at ordinary depth: 300-900 operations each, aligned runs of 1..700 bases"""
    rng = np.random.default_rng(seed)
    ref = _bases(rng, L, "ACGTACGTACGTACGTACGTACGTN")
    reads = []
    for i in range(n_reads):
        plant = [PLANTED_RUNS[(3 * i + t) % len(PLANTED_RUNS)] for t in range(3)]
        if i % 5 == 2:
            plant.append(700 if i == 2 else int(rng.integers(300, 701)))
        plant_at = None
        if i % 8 == 0:                               # the run's last base is operation 63 / 127, a P and then the I behind the batch boundary
            plant_at = {64: [("P", 1), ("I", 2)], 128: [("P", 1), ("I", 3)]}
        elif i % 8 == 4:                             # two P in a row, and a deletion behind a P
            plant_at = {64: [("P", 1), ("P", 2), ("I", 1)], 128: [("P", 1), ("D", 2)]}
        lead = [("S", 5)] if i % 3 == 1 else ([("H", 7)] if i % 3 == 2 else [])
        cigar = _long_cigar(rng, int(rng.integers(160, 421)), int(rng.integers(4000, 8001)), plant, plant_at, lead)
        if i % 7 == 3:
            cigar.append(("S", 9))
        assert 300 <= len(cigar) <= 900, len(cigar)
        flag = 16 * int(rng.random() < 0.5) | (256 if i % 29 == 3 else 0) | (1024 if i % 31 == 4 else 0)
        reads.append(_read(rng, "L%d" % i, flag, 0, int(rng.integers(0, L - ref_len_of(cigar) + 1)), cigar,
                           mapq=int(rng.choice([0, 3, 20, 60, 60, 60, 120, 255])), alphabet="ACGTACGTACGTN=RY", no_qual=i % 13 == 7,
                           cg_tag=i % 11 == 5))
    reads.sort(key=lambda r: r["pos"])
    edges, last = [], 0                              # intervals that are exactly one planted long run each, disjoint
    for a, n in sorted(run for r in reads if accepted(r, 0) for run in aligned_runs(r) if run[1] in PLANTED_RUNS or run[1] > 256):
        if a >= last:
            edges.append((a, a + n))
            last = a + n
    mid = reads[len(reads) // 2]
    cut = (mid["pos"] + 1500, mid["pos"] + 3500)     # 1-based, both ends inside that read
    regions = [(0, 1, L, None, 8000), (0, 1, L, _windows(100, L - 100, 33, 211), 8000), (0, 1, L, _windows(50, L, 1, 37), 8000),
               (0, 1, L, edges, 8000), (0, cut[0], cut[1], None, 8000)]
    return Case([("chrL", L)], [ref], reads, regions, dict(cigar_figures(reads, 0), n_run_edges=len(edges)))


DEEP_REGIONS = ("whole", "bed33")


def deep_long_reads(seed=102, n_reads=150, L=5000):
    """every read open at the last read's start: the open ends take more than two passes of 64, the CIGARs more than one batch"""
    rng = np.random.default_rng(seed)
    ref = _bases(rng, L)
    reads = []
    for i in range(n_reads):
        plant = [PLANTED_RUNS[i % len(PLANTED_RUNS)]]
        cigar = _long_cigar(rng, int(rng.integers(52, 141)), int(rng.integers(2000, 3001)), plant,
                            {64: [("P", 1), ("I", 2)]} if i % 10 == 0 else None)
        assert 100 <= len(cigar) <= 300, len(cigar)
        reads.append(_read(rng, "d%d" % i, 16 * int(rng.random() < 0.5), 0, int(rng.integers(0, 1200)), cigar, alphabet="ACGTACGTN=",
                           no_qual=i % 17 == 5, cg_tag=i % 19 == 3))
        assert reads[-1]["pos"] + ref_len_of(cigar) <= L
    reads.sort(key=lambda r: r["pos"])
    regions = [(0, 1, L, None, 8000), (0, 1001, 4000, _windows(1000, 4000, 33, 97), 8000)]
    return Case([("chrD", L)], [ref], reads, regions, cigar_figures(reads, 0))


STACK_L, STACK_P = 1000, 500                          # P: the 1-based position every read of a stack covers


def stack(D, max_depth=8000, seed=103):
    """D reads of 40 reference bases that all cover position P: equal starts and equal ends everywhere"""
    rng = np.random.default_rng(seed + D)
    ref = _bases(rng, STACK_L)
    p0 = STACK_P - 1
    carriers = set(range(3, D, max(1, D // 9)))
    reads = []
    for i in range(D):
        s = p0 - 39 + (i * 40) // D
        k = p0 - s                                   # P is base k of the read
        cigar = [("M", 40)]
        if i in carriers and k <= 30:
            n = 1 + i % 3
            cigar = [("M", k + 1), ("I", n), ("M", 39 - k)] if i % 2 else [("M", k + 1), ("D", n), ("M", 39 - k - n)]
        assert ref_len_of(cigar) == 40
        reads.append(_read(rng, "s%d" % i, 16 * (i % 3 == 1), 0, s, cigar))
    figs = dict(D=D, P=STACK_P, open_at_last=open_at_starts(reads, 0)[-1], n_carriers=sum(len(r["cigar"]) > 1 for r in reads))
    # the second region asks for the positions behind P only: the reads open at the last read's start stay D - 1, no column has D reads
    regions = [(0, 1, STACK_L, None, max_depth), (0, 1, STACK_L, [(STACK_P, STACK_P + 20)], max_depth)]
    return Case([("chrS", STACK_L)], [ref], reads, regions, figs)


KEYS_P = 120


def _key_specs(rng):
    """distinct indel keys (strand, anchor base, kind, length or inserted bases), the special ones first"""
    over = [_bases(rng, 61), _bases(rng, 70)]
    first = [(0, "A", "I", "AC"), (16, "A", "I", "AC"),            # anchors that differ in case only: two keys, one merged group
             (0, "C", "I", "ANC"), (0, "G", "D", 3), (16, "G", "D", 3), (0, "T", "D", 3),      # deletions merge by length
             (0, "A", "I", over[0]), (16, "C", "D", 70), (0, "N", "I", "G"), (16, "N", "D", 1), (0, "T", "D", 60), (16, "T", "D", 59)]
    rest = [(st, an, kind, v) for st in (0, 16) for an in "ACGTN"
            for kind, vals in (("I", ["A", "C", "G", "T", "AC", "CA", "GT", "TTT", "ANC", "ACGTA", "R", "NN"] + over), ("D", [1, 2, 3, 4, 5, 59, 60, 61, 70]))
            for v in vals]
    rest = [rest[i] for i in rng.permutation(len(rest))]
    return first + [s for s in rest if s not in first]


def keys(K, seed=104):
    """one column, position KEYS_P, with exactly K distinct indel keys, then 30 more carriers of keys already seen"""
    rng = np.random.default_rng(seed)
    L = 400
    ref = _bases(rng, L)
    specs = _key_specs(rng)[:K]
    assert len(set(specs)) == K
    pos = KEYS_P - 20

    def carrier(name, spec, eq_for_n=False):
        strand, anchor, kind, v = spec
        left, right = _bases(rng, 19), _bases(rng, 20)
        if kind == "I":
            ins = v.replace("N", "=") if eq_for_n else v           # '=' and N in inserted bases are one key
            return _read(rng, name, strand, 0, pos, [("M", 20), ("I", len(v)), ("M", 20)], seq=left + anchor + ins + right)
        return _read(rng, name, strand, 0, pos, [("M", 20), ("D", v), ("M", 20)], seq=left + anchor + right)
    reads = [_read(rng, "p%d" % i, 16 * (i & 1), 0, pos, [("M", 41)]) for i in range(3)]
    reads += [carrier("k%d" % i, s) for i, s in enumerate(specs)]
    again = [K - 1, 0, 2, K - 1, 1] + [int(x) for x in rng.integers(0, K, size=25)]     # the last-opened key among them
    reads += [carrier("a%d" % i, specs[k], eq_for_n=bool(i & 1) or k == 2) for i, k in enumerate(again)]
    reads += [_read(rng, "q%d" % i, 16 * (i & 1), 0, pos, [("M", 41)]) for i in range(2)]
    return Case([("chrK", L)], [ref], reads, [(0, 1, L, None, 8000)], dict(K=K, P=KEYS_P, depth=len(reads)))


def few(n, seed=105):
    """n reads that pass the filters among as many that do not (MAPQ below min_mq = 20, unmapped, secondary, supplementary flags,
    another contig)"""
    rng = np.random.default_rng(seed + n)
    refs = [("c0", 600), ("chrF", 2000)]
    ref_seqs = [_bases(rng, 600), _bases(rng, 2000)]
    reads = [_read(rng, "o%d" % i, 0, 0, 100 + 50 * i, [("M", 60)]) for i in range(3)]
    starts = sorted(int(x) for x in rng.integers(50, 1500, size=2 * n + 3))
    n_ok = 0
    for i, s in enumerate(starts):
        cigar = [("M", int(rng.integers(20, 90))), (str(rng.choice(["I", "D"])), int(rng.integers(1, 4))), ("M", int(rng.integers(20, 90))),
                 ("D", 2), ("=", int(rng.integers(5, 60)))]
        ok = i % 2 == 1 and n_ok < n
        n_ok += ok
        flag, mapq = 16 * int(rng.random() < 0.5), int(rng.choice([20, 60]))
        if not ok:
            kind = i % 4 if i % 2 == 0 else 0
            flag |= {0: 0, 2: 256}.get(kind, 0) | (2048 if i % 8 == 6 else 0) | (4 if i % 16 == 8 else 0)
            if kind == 0:
                mapq = 19
        reads.append(_read(rng, "f%d" % i, flag, 1, s, cigar, mapq=mapq))
    figs = dict(n=n, min_mq=20, n_accepted=sum(accepted(r, 1, 20) for r in reads), n_rejected=sum(r["ref"] == 1 and not accepted(r, 1, 20) for r in reads))
    return Case(refs, ref_seqs, reads, [(1, 1, 2000, None, 8000)], figs)


HUGE_REGIONS = ("whole", "bed1", "middle")


def huge_cigar(seed=106, n_ops=70000):
    """one read of 70 000 operations - 1M, 1I, 1M, 1D in turn - which only the CG:B,I tag can hold, among a few ordinary reads"""
    rng = np.random.default_rng(seed)
    cigar = [("S", 3)] + [(("M", "I", "M", "D")[k & 3], 1) for k in range(n_ops - 1)]
    assert len(cigar) == n_ops and cigar[-1][0] == "M"
    L = 500 + ref_len_of(cigar) + 700
    ref = _bases(rng, L)
    small = [("M", 50), ("I", 2), ("M", 60), ("D", 3), ("X", 40)]
    reads = [_read(rng, "h%d" % i, 16 * (i & 1), 0, s, small) for i, s in enumerate(
        [100, 450, 500, 501, 20000, 20100, 30000, 500 + ref_len_of(cigar) - 60, 500 + ref_len_of(cigar) + 100])]
    reads.insert(3, _read(rng, "huge", 0, 0, 500, cigar, alphabet="ACGTN=", cg_tag=True))
    reads.sort(key=lambda r: r["pos"])
    regions = [(0, 1, L, None, 8000), (0, 401, 8000, _windows(400, 8000, 1, 37), 8000), (0, 20001, 20600, None, 8000)]
    return Case([("chrH", L)], [ref], reads, regions, dict(n_ops=n_ops, max_ops=max(len(r["cigar"]) for r in reads)))


STACK_DEPTHS = (64, 65, 128, 129, 1024, 1025, 2048)      # both sides of every doubling of live_cap that a column of <= 2048 reads meets
FEW_NS = (1, 2, 7, 8, 9)
KEY_COUNTS = (63, 64)
REGION_LABELS = dict(long_reads=LONG_REGIONS, deep_long_reads=DEEP_REGIONS, huge_cigar=HUGE_REGIONS)


@functools.lru_cache(maxsize=None)
def case(name):
    """'long_reads', 'deep_long_reads', 'huge_cigar', 'few<n>', 'stack<D>', 'stack<D>cap<max_depth>', 'keys<K>': built once per process"""
    if name in REGION_LABELS:
        c = globals()[name]()
        assert len(c.regions) == len(REGION_LABELS[name])
        return c
    if name.startswith("few"):
        return few(int(name[3:]))
    if name.startswith("keys"):
        return keys(int(name[4:]))
    assert name.startswith("stack"), name
    D, _, cap = name[5:].partition("cap")
    return stack(int(D), max_depth=int(cap) if cap else 8000)


def on_device_cases():
    """(case name, region index, test id) of every case the device has to take itself"""
    out = [(n, i, "%s-%s" % (n, lab)) for n in ("long_reads", "deep_long_reads", "huge_cigar") for i, lab in enumerate(REGION_LABELS[n])]
    out += [("few%d" % n, 0, "few%d" % n) for n in FEW_NS]
    out += [("stack%d" % D, 0, "stack%d" % D) for D in STACK_DEPTHS]
    out += [("stack200cap200", 0, "stack200cap200")]
    out += [("keys%d" % K, 0, "keys%d" % K) for K in KEY_COUNTS]
    return out


def stack_bam_name(name):
    """the stacks of one depth differ in the cap only: one BAM"""
    return name.partition("cap")[0]


class Bams(object):
    """the cases' BAM files, each written once (into a directory of tmp_path_factory)"""

    def __init__(self, root):
        self.root, self.done = root, {}

    def __call__(self, name):
        name = stack_bam_name(name)
        if name not in self.done:
            c = case(name)
            path = str(self.root / (name + ".bam"))
            big = sum(len(r["seq"]) for r in c.reads) > 200000
            write_bam(path, c.refs, c.reads, block_payload=60000 if big else 1500)
            self.done[name] = path
        return self.done[name]


def pack_arrays(pack):
    a = {k: v.copy() for k, v in pack.numpy().items()}
    a["keys"] = [pack.key_string(k) for k in range(pack.n_keys)]
    return a


def host_pack(bam, c, region):
    from clairs_to_amd.pack import ColumnPack
    ri, start, end, bed, max_depth = region
    return pack_arrays(ColumnPack.from_bam(bam, c.refs[ri][0], start, end, c.ref_seqs[ri], 1, bed=bed, min_mq=c.figs.get("min_mq", 0),
                                           max_depth=max_depth))


def naive_pack(c, region):
    from clairs_to_amd.pack import ColumnPack
    ri, start, end, bed, max_depth = region
    text = mpileup_rows(c.reads, ri, c.refs[ri][0], start, end, bed=bed, min_mq=c.figs.get("min_mq", 0), max_depth=max_depth,
                        ref_seq=c.ref_seqs[ri], ref_start=1)
    return pack_arrays(ColumnPack.from_mpileup(text, c.ref_seqs[ri], 1))


def assert_same(got, want, what=""):
    for k in ARRAYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s %s" % (k, what))
    assert got["keys"] == want["keys"], what


def restrict(a, col_pos):
    """the pack `a` cut down to the columns of the positions col_pos, which have to be a contiguous run of its columns"""
    idx = np.searchsorted(a["col_pos"], col_pos)
    assert len(idx) and idx[-1] < len(a["col_pos"]) and (a["col_pos"][idx] == col_pos).all() and (np.diff(idx) == 1).all()
    c0, c1 = int(idx[0]), int(idx[-1]) + 1
    e0, e1, k0, k1 = int(a["col_off"][c0]), int(a["col_off"][c1]), int(a["key_off"][c0]), int(a["key_off"][c1])
    return dict(col_pos=a["col_pos"][c0:c1], col_ref=a["col_ref"][c0:c1], col_off=a["col_off"][c0:c1 + 1] - e0,
                key_off=a["key_off"][c0:c1 + 1] - k0, entries=a["entries"][e0:e1], key_meta=a["key_meta"][k0:k1],
                key_group=a["key_group"][k0:k1], keys=a["keys"][k0:k1])


def depth_at(a, pos1):
    """entries in the column of 1-based position pos1 (0: no such column)"""
    hit = np.nonzero(a["col_pos"] == pos1)[0]
    return int(a["col_off"][hit[0] + 1] - a["col_off"][hit[0]]) if len(hit) else 0


def assert_reach(name, region_i, host):
    """the case is the case it claims to be: from the builder's figures and the host reader's pack of the region"""
    f = case(name).figs
    depth, nkeys = np.diff(host["col_off"]), np.diff(host["key_off"])
    if name == "long_reads":
        assert f["max_ops"] > 128 and f["n_over_64"] >= 50 and f["longest_run"] > 256
        assert set(PLANTED_RUNS) <= f["run_lengths"] and 1 in f["run_lengths"] and 700 in f["run_lengths"]
        assert f["n_p_at_boundary"] >= 3 and f["n_cg"] >= 3 and f["n_run_edges"] >= 20
        assert len(host["col_pos"]) > 0 and nkeys.max() >= 2
        if region_i == 0:
            assert 30 <= depth.max() < 64 and len(depth) > 19000 and (host["key_meta"] & 8).any()      # overlong keys are there
    elif name == "deep_long_reads":
        assert f["min_ops"] > 64 and f["n_p_at_boundary"] >= 3
        assert 128 <= f["max_open"] < 256 and depth.max() == f["max_open"] + 1                          # live_cap = 256
    elif name == "huge_cigar":
        assert f["max_ops"] == f["n_ops"] > 65535 and len(host["col_pos"]) > 0
        if region_i == 0:
            assert len(host["keys"]) > f["n_ops"] // 2 - 10                                            # every M of it carries an indel
    elif name.startswith("few"):
        assert f["n_accepted"] == f["n"] and f["n_rejected"] >= f["n"] and depth.max() <= f["n"] and depth.sum() > 0
    elif name.startswith("keys"):
        assert nkeys.max() == f["K"] and depth_at(host, f["P"]) == f["depth"]
        assert (host["key_meta"] & 8).any() and len(set(host["key_group"].tolist())) < f["K"]
    else:
        assert name.startswith("stack")
        assert f["open_at_last"] == f["D"] - 1 and f["n_carriers"] >= 4
