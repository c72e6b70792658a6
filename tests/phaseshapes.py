"""Test-only: one generated BAM that takes the kernels of csrc/phase.hip past their first trip - reads of more than 64 and more than 128
CIGAR operations with sites planted at the pass boundaries, more than 64 sites under one operation, reads of more than 64 observations,
more than 70 phase blocks with ties and threshold votes, letters that observe nothing, and a second contig whose BGZF block a test
damages.  Everything is built from bamutil read dicts and checked with phaseutil's naive restatement (check_case) before a test uses it.
The sites are held in named groups (GROUPS); reads and reference are all A unless a read says otherwise, REF is A and ALT is C at
every site but the `letters` group's."""
import functools
import shutil

import numpy as np

import bamutil
import phaseutil as pu
from bamutil import CONSUMES_QUERY, CONSUMES_REF, ref_len_of

SEED = 20261021
CTG, CTG2 = "q1", "q2"
REFS = [(CTG, 30000), (CTG2, 3000)]
BLOCK_PAYLOAD = 331                            # records straddle blocks, the long ones several
CHUNK_BYTES = "4000"                           # CTO_PHASE_CHUNK_BYTES that cuts q1 into at least MIN_CUT_CHUNKS chunks at levels 0 and 6
MIN_CUT_CHUNKS = 4
LINK_SPANS = (1, 8, 63, 64)
GEOM_BYTES = "300"                             # ... and one that cuts the few hundred bases of `geom` as often, inside its adjacent sites too
# (group, link span, CTO_PHASE_CHUNK_BYTES) of the runs that are cut into chunks
CUT_CASES = (("all", 8, CHUNK_BYTES), ("all", 64, CHUNK_BYTES), ("ops", 8, CHUNK_BYTES), ("geom", 63, GEOM_BYTES))
N_DENSE, N_SPARSE = 210, 5                     # sites of `geom`: adjacent ones, and the others
GROUPS = ("few", "ops", "geom", "letters", "blocks")
N_ISLANDS = 72
ISLAND_STEP = 250
BLOCKS_AT = 9000
BIG = (10, 12, 14, 16, 18, 20, 22, 24)         # islands of twelve sites with eight reads: the threshold reads' blocks
FIVE = range(28, 46)                           # islands of five sites: the tie read's and its neighbours'
N_Q2, Q2_DAMAGED = 16, 12                      # reads on q2 (3 kB records); the damaged block starts behind this one's end
UNPHASED = (50, 51)                            # islands of eight sites whose sites 3, 4, 5 stay unphased


# ------------------------------------------------------------------------------------------ geometry of a read
def op_at(read, pos0):
    """(operation index, offset inside the operation, query index or None) of 0-based reference position pos0 inside the read's span"""
    rp, qp = read["pos"], 0
    for k, (op, n) in enumerate(read["cigar"]):
        if op in CONSUMES_REF:
            if pos0 < rp + n:
                return k, pos0 - rp, (qp + pos0 - rp) if op in "M=X" else None
            rp += n
        if op in CONSUMES_QUERY:
            qp += n
    raise AssertionError("position outside the read")


def op_start(read, k):
    """0-based reference position of the first base of operation k"""
    return read["pos"] + ref_len_of(read["cigar"][:k])


def end_of(read):
    return read["pos"] + ref_len_of(read["cigar"])


def _chain(n_ops, lead=(), seps="IDNP", at=None):
    """`lead`, then an aligned run of 3 (M, =, X in turn) and a separator of 2 (`seps` in turn) alternately, n_ops operations in all;
    at = {operation index: (op, n)} overrides; a separator at the end becomes X3"""
    ops, k = list(lead), 0
    while len(ops) < n_ops:
        if (len(ops) - len(lead)) % 2 == 0:
            ops.append(("M=X"[(len(ops) // 2) % 3], 3))
        else:
            ops.append((seps[k % len(seps)], 2))
            k += 1
    for i, o in (at or {}).items():
        ops[i] = o
    if ops[-1][0] not in "M=X":
        ops[-1] = ("X", 3)
    return ops


# ------------------------------------------------------------------------------------------ the case
class _Build(object):
    def __init__(self):
        self.rng = np.random.default_rng(SEED)
        self.sites = {}                        # 1-based position -> dict(ref, alt, group, h1: the allele haplotype 1's reads carry)
        self.named = {}                        # name of a planted site -> 1-based position
        self.reads = []

    def site(self, group, pos1, h1=0, ref="A", alt="C", name=None):
        assert pos1 not in self.sites, pos1
        self.sites[pos1] = dict(ref=ref, alt=alt, group=group, h1=h1)
        if name:
            assert name not in self.named, name
            self.named[name] = pos1
        return pos1

    def read(self, name, start, cigar, hap=None, bases=None, fill="A", flag=0, mapq=60, ref=0, **kw):
        """hap 1 / 2: the read carries that haplotype's letter at every site under an aligned base; bases = {1-based position: letter}
        overrides; every other base is `fill` (one letter, or several to draw from)"""
        r = dict(name=name, flag=flag, ref=ref, pos=start, mapq=mapq, cigar=list(cigar), hap=hap, bases=dict(bases or {}), fill=fill, **kw)
        self.reads.append(r)
        return r

    def cover(self, tag, lo, hi, length, step):
        """ordinary reads of one M operation over [lo, hi), the two haplotypes in turn"""
        for i, s in enumerate(range(lo, hi, step)):
            self.read("%s%d" % (tag, i), s, [("M", length)], hap=1 + (i & 1))

    def finish(self):
        assert len(set(r["name"] for r in self.reads)) == len(self.reads)
        for r in self.reads:
            ql = sum(n for op, n in r["cigar"] if op in CONSUMES_QUERY)
            fill = r.pop("fill")
            seq = [fill] * ql if len(fill) == 1 else [str(c) for c in self.rng.choice(list(fill), size=ql)]
            hap, bases = r.pop("hap"), r.pop("bases")
            rp, qp = r["pos"], 0
            for op, n in r["cigar"]:
                if op in "M=X":
                    for k in range(n):
                        s = self.sites.get(rp + k + 1)
                        if s is not None and r["ref"] == 0 and hap:
                            seq[qp + k] = (s["ref"], s["alt"])[s["h1"] if hap == 1 else 1 - s["h1"]].upper()
                        if rp + k + 1 in bases:
                            seq[qp + k] = bases[rp + k + 1]
                if op in CONSUMES_REF:
                    rp += n
                if op in CONSUMES_QUERY:
                    qp += n
            r["seq"], r["qual"] = "".join(seq), [30] * ql
        self.reads.sort(key=lambda r: (r["ref"], r["pos"]))      # stable


def _few(b):
    """three sites: a link span of 64 is far more than there are sites"""
    for p, h in ((521, 0), (541, 1), (561, 1)):
        b.site("few", p, h1=h)
    b.cover("f", 400, 700, 200, 50)


def _ops(b):
    """A. reads of 65 .. 362 operations, one per stretch so that a read's planted sites are all the sites it covers"""
    S = lambda name, pos0, h1: b.site("ops", pos0 + 1, h1=h1, name=name)
    many = dict(fill="GT")                                        # neither REF nor ALT anywhere but at the planted sites
    # 65 operations: S2, aligned runs at the odd indices up to 63, X3 as operation 64.  Its last site is the first base of operation 64
    r = b.read("ops65", 1000, _chain(65, lead=[("S", 2)]), hap=1, **many)
    S("ops65_first_base", op_start(r, 1), 0)
    S("ops65_op31", op_start(r, 31) + 1, 1)
    S("ops65_op63_last", op_start(r, 63) + 2, 1)
    S("ops65_op64_first", op_start(r, 64), 0)
    # 129 operations on the reverse strand: I2 as operation 64 (lane 0 of the second pass), its last site the first base of operation 128
    r = b.read("ops129", 1300, _chain(129, lead=[("S", 2)], at={64: ("I", 2)}), hap=2, flag=16, **many)
    S("ops129_op1", op_start(r, 1) + 1, 1)
    S("ops129_op63_last", op_start(r, 63) + 2, 0)
    S("ops129_behind_i64", op_start(r, 65), 1)
    S("ops129_op65", op_start(r, 65) + 2, 0)
    S("ops129_op127_last", op_start(r, 127) + 2, 1)
    S("ops129_op128_first", op_start(r, 128), 0)
    # 150 operations under the long-CIGAR placeholder: D2 as operation 64, N2 as operation 128
    r = b.read("ops150cg", 1700, _chain(150, lead=[("S", 3)], at={64: ("D", 2), 128: ("N", 2)}), hap=1, cg_tag=True, **many)
    S("ops150_op63_last", op_start(r, 63) + 2, 0)
    S("ops150_in_d64", op_start(r, 64), 1)
    S("ops150_op65_first", op_start(r, 65), 1)
    S("ops150_op127", op_start(r, 127) + 1, 0)
    S("ops150_in_n128", op_start(r, 128) + 1, 1)
    S("ops150_op129_first", op_start(r, 129), 0)
    S("ops150_last_base", end_of(r) - 1, 1)
    # 131 operations: N2 as operation 64, D2 as operation 128
    r = b.read("ops131", 2100, _chain(131, lead=[("H", 5)], at={64: ("N", 2), 128: ("D", 2)}), hap=2, **many)
    S("ops131_op1", op_start(r, 1), 0)
    S("ops131_in_n64", op_start(r, 64), 1)
    S("ops131_op65_first", op_start(r, 65), 0)
    S("ops131_in_d128", op_start(r, 128) + 1, 0)
    S("ops131_op129_first", op_start(r, 129), 1)
    S("ops131_op130", op_start(r, 130) + 1, 1)
    # 362 operations: a site under the first and the last aligned run of every 64 operations
    r = b.read("ops362", 2500, _chain(362, lead=[("H", 4), ("S", 2)]), hap=1, **many)
    for k0 in range(0, 362, 64):
        al = [k for k in range(k0, min(k0 + 64, 362)) if r["cigar"][k][0] in "M=X"]
        S("ops362_run%d_first" % (k0 // 64), op_start(r, al[0]) + (k0 // 64) % 3, (k0 // 64) & 1)
        S("ops362_run%d_last" % (k0 // 64), op_start(r, al[-1]) + (k0 // 64 + 1) % 3, 1 - ((k0 // 64) & 1))
    # 140 operations whose last site lies in the first 64: the walk ends early.  Behind that site no site for a few hundred bases
    r = b.read("ops140_early", end_of(r) + 80, _chain(140, lead=[("S", 1)]), hap=2, **many)
    for k in (1, 21, 41, 61):
        S("ops140_op%d" % k, op_start(r, k) + k % 3, (k >> 1) & 1)
    # 220 operations that start in that stretch: the first site lies behind operation 128, two whole passes see none
    r2 = b.read("ops220_late", op_start(r, 70), _chain(220, lead=[("H", 3), ("S", 4)]), hap=1, **many)
    for k in (130, 150, 170, 190, 210):
        S("ops220_op%d" % k, op_start(r2, k) + k % 3, (k // 10) & 1)
    S("ops220_last_base", end_of(r2) - 1, 0)
    b.cover("o", 600, end_of(r2) + 100, 500, 125)


def _geom(b):
    """B and D. 210 adjacent sites under single operations; reads that begin and end on sites; a read between two sites; one aligned base"""
    for p in range(5001, 5211):
        b.site("geom", p, h1=int(b.rng.integers(0, 2)))
    b.read("long_m1", 4900, [("M", 400)], hap=1)
    b.read("long_m2", 4950, [("S", 3), ("M", 400)], hap=2)
    for name, start, n, hap in (("obs64", 5000, 64, 1), ("obs65", 5010, 65, 2), ("obs128", 5020, 128, 1), ("obs129", 5030, 129, 2),
                                ("obs200", 5005, 200, 1)):
        b.read(name, start, [("M", n)], hap=hap)                  # first base on a site, last base on a site, the site at pos == end not covered
    b.read("obs140_gappy", 5000, [("M", 210)], hap=2, bases={p: "G" for p in range(5001, 5211, 3)})
    b.cover("g", 4700, 5300, 300, 75)
    for name, p, h in (("gap_lo", 5401, 0), ("gap_hi", 5501, 1), ("ends_first", 5601, 1), ("ends_last", 5650, 0), ("one_base", 5701, 1)):
        b.site("geom", p, h1=h, name=name)
    b.read("between", 5420, [("M", 60)], hap=1)                    # enters, and covers no site
    b.read("ends", 5600, [("M", 50)], hap=1)
    b.read("ends_short", 5600, [("M", 49)], hap=2)                 # site 5650 is its pos == end
    b.read("one_m_even", 5700, [("S", 5), ("I", 3), ("M", 1), ("I", 2), ("S", 4)], hap=2, fill="GT")
    b.read("one_m_odd", 5700, [("S", 5), ("M", 1), ("S", 3)], hap=1, fill="GT")
    b.cover("h", 5300, 5800, 200, 50)


LETTER_SITES = [("A", "C"), ("a", "C"), ("A", "c"), ("g", "t"), ("N", "C"), ("A", "R"), ("A", "N"), ("A", "C"), ("T", "G"), ("n", "c"), ("A", "C"),
                ("C", "A")]


def _letters(b):
    """C. lower-case letters, REF N with a real ALT, ALTs that are no base; reads with N, IUPAC codes, `=` and a third allele at sites"""
    pos = [7041 + 40 * k for k in range(len(LETTER_SITES))]
    for k, (ref, alt) in enumerate(LETTER_SITES):
        b.site("letters", pos[k], h1=k & 1, ref=ref, alt=alt, name="letters%d" % k)
    b.cover("l", 6800, 7700, 400, 50)
    b.read("iupac", 7020, [("M", 500)], bases=dict(zip(pos, "RACT=RNNA=MA")))
    b.read("all_equals", 7030, [("M", 500)], fill="=")
    b.read("all_n", 7035, [("M", 500)], fill="N")


def island_start(i):
    return BLOCKS_AT + ISLAND_STEP * i


def island_size(i):
    return 12 if i in BIG else 5 if i in FIVE else 8 if i in UNPHASED else 3


def island_site(i, j):
    """1-based position of site j of island i"""
    return island_start(i) + 21 + 10 * j


def _blocks(b):
    """E. islands of sites, each under reads of its own, joined by at most one read that observes no island's first site: every island is
    a phase block.  Haplotype 1 of a block is the one with REF at its first site."""
    bit = {}
    for i in range(N_ISLANDS):
        n = island_size(i)
        for j in range(n):
            bit[i, j] = int(b.rng.integers(0, 2))
            b.site("blocks", island_site(i, j), h1=bit[i, j])
        for k in range(8 if i in BIG else 4):
            over = {island_site(i, j): "AC"[(k >> 1) & 1] for j in (3, 4, 5)} if i in UNPHASED else None    # half of each haplotype's reads
            b.read("i%d_%d" % (i, k), island_start(i) + 2 * k, [("M", 10 * n + 40)], hap=1 + (k & 1), bases=over)
    letter = lambda i, j, hp: "AC"[(bit[i, j] ^ bit[i, 0]) ^ (hp - 1)]          # the base that votes for haplotype hp of island i at site j

    def voter(name, i0, i1, votes):
        """a read over islands i0 .. i1 that observes exactly the sites of votes = [(island, site, haplotype)]"""
        assert all(j > 0 for i, j, _ in votes) or i0 == i1
        b.read(name, island_start(i0) + 10, [("M", island_start(i1) - island_start(i0) + 150)], fill="G",
               bases={island_site(i, j): letter(i, j, hp) for i, j, hp in votes})
    voter("t35_h1", 10, 10, [(10, j, hp) for j, hp in zip((1, 3, 4, 6, 9), (1, 2, 1, 2, 1))])
    voter("t35_h2", 12, 12, [(12, j, hp) for j, hp in zip((0, 2, 5, 7, 11), (2, 1, 2, 1, 2))])
    voter("t610_h1", 14, 14, [(14, j, hp) for j, hp in zip(range(1, 11), (1, 2, 1, 1, 2, 1, 2, 1, 2, 1))])
    voter("t610_h2", 16, 16, [(16, j, hp) for j, hp in zip(range(2, 12), (2, 2, 1, 1, 2, 1, 2, 2, 1, 2))])
    voter("t59_h1", 18, 18, [(18, j, hp) for j, hp in zip(range(1, 10), (1, 2, 1, 2, 1, 2, 1, 2, 1))])
    voter("t59_h2", 20, 20, [(20, j, hp) for j, hp in zip(range(3, 12), (2, 1, 2, 1, 2, 1, 2, 1, 2))])
    voter("t12_a", 22, 22, [(22, 2, 1), (22, 7, 2)])
    voter("t12_b", 24, 24, [(24, 3, 2), (24, 5, 1)])
    voter("tie", 30, 34, [(30, 2, 2), (31, 1, 1), (31, 3, 1), (31, 4, 1), (32, 1, 2), (32, 2, 2), (33, 1, 2), (33, 2, 2), (33, 4, 2), (34, 3, 1)])
    voter("later", 38, 40, [(38, 1, 1), (38, 2, 1), (39, 3, 1), (40, 1, 2), (40, 2, 2), (40, 3, 2), (40, 4, 2)])
    voter("middle", 42, 44, [(42, 4, 2), (43, 1, 1), (43, 2, 1), (43, 4, 1), (44, 1, 2), (44, 3, 2)])
    b.read("only_unphased", island_site(50, 3) - 6, [("M", 30)])                # sites 3, 4, 5 of island 50 and no other
    voter("both_sides", 51, 51, [(51, 1, 1), (51, 2, 1), (51, 4, 1), (51, 6, 1), (51, 7, 1)])


# what the rules make of the planted reads, written out by hand: read -> (HP, island whose first site is the PS, or None)
HAND_TAGS = {"t35_h1": (1, 10), "t35_h2": (2, 12), "t610_h1": (1, 14), "t610_h2": (2, 16), "t59_h1": (0, None), "t59_h2": (0, None),
             "t12_a": (0, None), "t12_b": (0, None),
             "tie": (1, 31),                                         # 1, 3, 2, 3, 1 votes in islands 30 .. 34: the lower of the two threes
             "later": (2, 40), "middle": (1, 43), "only_unphased": (0, None), "both_sides": (1, 51)}
# (votes for haplotype 1, for haplotype 2) in the read's best block
HAND_VOTES = {"t35_h1": (3, 2), "t35_h2": (2, 3), "t610_h1": (6, 4), "t610_h2": (4, 6), "t59_h1": (5, 4), "t59_h2": (4, 5), "t12_a": (1, 1),
              "t12_b": (1, 1)}
# observations by planted site name and allele: `ops65` follows haplotype 1, `ops129` haplotype 2
HAND_OBS = {"ops65": [("ops65_first_base", 0), ("ops65_op31", 1), ("ops65_op63_last", 1), ("ops65_op64_first", 0)],
            "ops129": [("ops129_op1", 0), ("ops129_op63_last", 1), ("ops129_behind_i64", 0), ("ops129_op65", 1), ("ops129_op127_last", 0),
                       ("ops129_op128_first", 1)],
            "ops150cg": [("ops150_op63_last", 0), ("ops150_op65_first", 1), ("ops150_op127", 0), ("ops150_op129_first", 0),
                         ("ops150_last_base", 1)],               # nothing under the D and the N
            "ops131": [("ops131_op1", 1), ("ops131_op65_first", 1), ("ops131_op129_first", 0), ("ops131_op130", 0)]}
# the planted sites under a D or an N: they observe nothing
UNDER_D_N = {"ops150cg": ["ops150_in_d64", "ops150_in_n128"], "ops131": ["ops131_in_n64", "ops131_in_d128"]}
# planted site -> (read, operation index, offset in the operation, the operation's letter or None for any of M = X)
PLANTED_OPS = {"ops65_op63_last": ("ops65", 63, 2, None), "ops65_op64_first": ("ops65", 64, 0, "X"),
               "ops129_op63_last": ("ops129", 63, 2, None), "ops129_behind_i64": ("ops129", 65, 0, None), "ops129_op65": ("ops129", 65, 2, None),
               "ops129_op127_last": ("ops129", 127, 2, None), "ops129_op128_first": ("ops129", 128, 0, "X"),
               "ops150_op63_last": ("ops150cg", 63, 2, None), "ops150_in_d64": ("ops150cg", 64, 0, "D"), "ops150_op65_first": ("ops150cg", 65, 0, None),
               "ops150_in_n128": ("ops150cg", 128, 1, "N"), "ops150_op129_first": ("ops150cg", 129, 0, None),
               "ops131_in_n64": ("ops131", 64, 0, "N"), "ops131_op65_first": ("ops131", 65, 0, None), "ops131_in_d128": ("ops131", 128, 1, "D"),
               "ops131_op129_first": ("ops131", 129, 0, None)}
N_OPS = {"ops65": 65, "ops129": 129, "ops150cg": 150, "ops131": 131, "ops362": 362, "ops140_early": 140, "ops220_late": 220}
N_OBS = {"obs64": 64, "obs65": 65, "obs128": 128, "obs129": 129, "obs200": 200, "obs140_gappy": 140, "long_m1": 210, "long_m2": 210,
         "between": 0, "ends": 2, "ends_short": 1, "one_m_even": 1, "one_m_odd": 1, "all_equals": 0, "all_n": 0}


@functools.lru_cache(maxsize=None)
def _built():
    b = _Build()
    for part in (_few, _ops, _geom, _letters, _blocks):
        part(b)
    for i in range(N_Q2):                                          # F. the other contig: its blocks lie behind q1's in the file
        b.read("z%d" % i, 100 + 50 * i, [("M", 2000)], ref=1)
    b.finish()
    sites = {g: [(p, s["ref"], s["alt"]) for p, s in sorted(b.sites.items()) if s["group"] == g] for g in GROUPS}
    sites["all"] = [(p, s["ref"], s["alt"]) for p, s in sorted(b.sites.items())]
    return dict(reads=b.reads, sites=sites, named=dict(b.named), by_name={r["name"]: i for i, r in enumerate(b.reads)})


@functools.lru_cache(maxsize=None)
def case():
    """dict(reads (bamutil dicts, in file order), sites {group: [(pos, REF, ALT)]} with "all", named {site name: pos}, by_name {read name:
    index into reads}); checked by check_case"""
    check_case(_built())
    return _built()


def site_index(group, name_or_pos):
    """the index of a planted site (by name) or of a 1-based position among one group's sites"""
    c = _built()
    return [s[0] for s in c["sites"][group]].index(c["named"].get(name_or_pos, name_or_pos))


@functools.lru_cache(maxsize=None)
def _observed(group):
    c = _built()
    ent = pu.entered(c["reads"], 0, c["sites"][group])
    return ent, [pu.observations(c["reads"][i], c["sites"][group]) for i in ent]


@functools.lru_cache(maxsize=None)
def expected(group, K):
    """phaseutil.naive over one group's sites (or "all"), with `block` per site and `names` of the entered reads; computed once, shared
    by every test (read-only)"""
    c = _built()
    sites = c["sites"][group]
    ent, obs = _observed(group)
    link = pu.link_table(obs, len(sites), K)
    phase, ps, block = pu.phase_pass(link, sites, K)
    return dict(entered=ent, names=[c["reads"][i]["name"] for i in ent], obs=obs, link=link, phase=phase, ps=ps, block=block,
                tags=pu.assign(obs, phase, ps, block), n_blocks=max(block) + 1)


def votes_per_block(e, name):
    """[(block, h1, h2)] of one entered read, ascending"""
    out = {}
    for s, x in e["obs"][e["names"].index(name)]:
        if e["phase"][s] >= 0:
            out.setdefault(e["block"][s], [0, 0])[x ^ e["phase"][s]] += 1
    return [(blk, v[0], v[1]) for blk, v in sorted(out.items())]


def hand_tag(name):
    hp, island = HAND_TAGS[name]
    return (hp, island_site(island, 0) if hp else 0)


def check_case(c):
    """the generated case holds every edge the tests rely on (run once, when the case is built): bamutil and the naive rules only"""
    reads, by, named = c["reads"], c["by_name"], c["named"]
    R = lambda name: reads[by[name]]
    assert 300 <= len(reads) <= 500, len(reads)
    # ---- A: operation counts, the long-CIGAR placeholder, the reverse strand, the planted operations
    for name, n in N_OPS.items():
        assert len(R(name)["cigar"]) == n and len(bamutil.effective_cigar(R(name))) == n, name
    assert R("ops150cg").get("cg_tag") and len(bamutil._cigar_field(R("ops150cg"))) == 2 and R("ops129")["flag"] & 16
    for k, kind in (("ops129", "I"), ("ops150cg", "D"), ("ops131", "N")):
        assert R(k)["cigar"][64][0] == kind, k
    assert R("ops150cg")["cigar"][128][0] == "N" and R("ops131")["cigar"][128][0] == "D"
    parity = set()
    for site, (name, k, off, op) in PLANTED_OPS.items():
        got_k, got_off, q = op_at(R(name), named[site] - 1)
        assert (got_k, got_off) == (k, off) and R(name)["cigar"][k][0] in (op or "M=X") and (q is None) == (op in ("D", "N")), site
        parity.add(q is not None and q & 1)
    assert parity == {0, 1}                                         # both nibbles of a sequence byte
    assert op_at(R("ops129"), named["ops129_behind_i64"] - 1)[2] == sum(n for op, n in R("ops129")["cigar"][:65] if op in CONSUMES_QUERY)
    ops_sites = [s[0] for s in c["sites"]["ops"]]
    under = lambda r: [p for p in ops_sites if r["pos"] < p <= end_of(r)]
    for name, by_hand in HAND_OBS.items():                          # every site of its stretch is written out by hand, D and N aside
        assert set(named[s] for s, _ in by_hand) | set(named[s] for s in UNDER_D_N.get(name, [])) == set(under(R(name))), name
    assert max(under(R("ops65"))) == named["ops65_op64_first"] and max(under(R("ops129"))) == named["ops129_op128_first"]
    r = R("ops362")
    for k0 in range(0, 362, 64):                                    # a site in every run of 64 operations
        assert any(op_start(r, k0) < p <= op_start(r, min(k0 + 64, 362)) for p in ops_sites), k0
    early, late = R("ops140_early"), R("ops220_late")
    assert op_at(early, max(under(early)) - 1)[0] < 64 and end_of(early) - max(under(early)) > 100
    assert op_at(late, min(under(late)) - 1)[0] > 128 and min(under(late)) - 1 > end_of(early)
    assert min(under(late)) - max(under(early)) > 200               # the stretch without a site
    e = expected("ops", 8)
    for name, by_hand in HAND_OBS.items():
        assert e["obs"][e["names"].index(name)] == [(site_index("ops", s), x) for s, x in by_hand], name
    # ---- B, D: observation counts
    geom = [s[0] for s in c["sites"]["geom"]]
    assert geom[:N_DENSE] == list(range(geom[0], geom[0] + N_DENSE)) and len(geom) == N_DENSE + N_SPARSE and geom[N_DENSE] > geom[N_DENSE - 1] + 1
    e = expected("geom", 8)
    n_obs = {n: len(o) for n, o in zip(e["names"], e["obs"])}
    for name, n in N_OBS.items():
        if name in n_obs:
            assert n_obs[name] == n, (name, n_obs[name])
    assert set(k for k in N_OBS if not k.startswith("all_")) <= set(n_obs)
    assert sum(n > 64 for n in n_obs.values()) >= 8 and sum(n > 128 for n in n_obs.values()) >= 5
    assert named["gap_lo"] < R("between")["pos"] + 1 and end_of(R("between")) < named["gap_hi"]
    assert R("ends")["pos"] + 1 == named["ends_first"] and end_of(R("ends")) == named["ends_last"] == end_of(R("ends_short")) + 1
    assert ref_len_of(R("one_m_even")["cigar"]) == 1 and {op_at(R(k), named["one_base"] - 1)[2] & 1 for k in ("one_m_even", "one_m_odd")} == {0, 1}
    # ---- C: letters
    e = expected("letters", 8)
    n_obs = {n: len(o) for n, o in zip(e["names"], e["obs"])}
    assert n_obs["all_equals"] == 0 and n_obs["all_n"] == 0
    li = lambda k: site_index("letters", "letters%d" % k)
    assert e["obs"][e["names"].index("iupac")] == [(li(1), 0), (li(2), 1), (li(3), 1), (li(11), 1)]      # A at a, C at c, T at t, A as ALT
    seen = {s for o in e["obs"] for s, _ in o}
    assert li(4) in seen and li(9) in seen and li(5) in seen and li(6) in seen       # ... and the other allele of N / R sites is observed
    # ---- E: blocks, ties, thresholds
    for K in LINK_SPANS:
        e = expected("blocks", K)
        assert e["n_blocks"] >= max(70, N_ISLANDS), (K, e["n_blocks"])
        for name in HAND_TAGS:
            if K >= 4 or name not in ("only_unphased", "both_sides"):  # a short link span cannot see past the run: it opens blocks inside it
                assert e["tags"][e["names"].index(name)] == hand_tag(name), (K, name)
        for name, v in HAND_VOTES.items():
            votes = votes_per_block(e, name)
            assert len(votes) == 1 and votes[0][1:] == v, (K, name, votes)
        assert [h1 + h2 for _, h1, h2 in votes_per_block(e, "tie")] == [1, 3, 2, 3, 1]
        assert [(h1, h2) for _, h1, h2 in votes_per_block(e, "later")] == [(2, 0), (1, 0), (0, 4)]
        assert [h1 + h2 for _, h1, h2 in votes_per_block(e, "middle")] == [1, 3, 2]
        assert (K < 4 or votes_per_block(e, "only_unphased") == []) and len(e["obs"][e["names"].index("only_unphased")]) == 3
    e = expected("blocks", 8)
    bi = lambda i, j: site_index("blocks", island_site(i, j))
    for i in UNPHASED:
        assert [e["phase"][bi(i, j)] >= 0 for j in range(8)] == [True] * 3 + [False] * 3 + [True] * 2, i
        assert len({e["block"][bi(i, j)] for j in (0, 1, 2, 6, 7)}) == 1
    assert len(votes_per_block(e, "both_sides")) == 1 and len(e["obs"][e["names"].index("both_sides")]) == 5
    assert expected("blocks", 1)["n_blocks"] > e["n_blocks"]        # a link span of 1 cannot see past the unphased runs
    assert expected("few", 64)["n_blocks"] == 1 and len(c["sites"]["few"]) == 3
    assert len(c["sites"]["all"]) == sum(len(c["sites"][g]) for g in GROUPS) <= 900


# ------------------------------------------------------------------------------------------ the file
def write(path, level=6):
    """the case as a BAM with its index -> what bamutil.write_bam returns, with voff (the virtual offset of every read) and name_of"""
    c = case()
    info = bamutil.write_bam(str(path), REFS, c["reads"], block_payload=BLOCK_PAYLOAD, level=level)
    info["voff"] = pu.voffs_of(info)
    info["name_of"] = {v: r["name"] for v, r in zip(info["voff"], c["reads"])}
    return info


def damaged_block(info):
    """the index of a BGZF block that holds q2's records only, far behind q2's first record - where the host path stops - and within
    the 64 KiB behind q1's last record that a device chunk over the end of q1 inflates.  Written without compression that is some
    40 kB behind q1's end, which the byte range of a chunk over the front of q1 does not reach."""
    c = case()
    n1 = sum(r["ref"] == 0 for r in c["reads"])
    starts = [0]
    for s in info["block_sizes"]:
        starts.append(starts[-1] + s)
    k = next(i for i in range(len(info["block_sizes"])) if starts[i] >= info["record_spans"][n1 + Q2_DAMAGED][1])
    last_q1 = max(i for i in range(len(info["block_sizes"])) if starts[i] < info["record_spans"][n1 - 1][1])
    assert k + 1 < len(info["block_sizes"]) and info["block_offsets"][k + 1] - info["block_offsets"][last_q1] < 60000
    return k


def write_damaged(src, dst, info):
    """a copy of the BAM `src` with one bit of the CRC-32 of damaged_block() flipped, and its index"""
    raw = bytearray(open(str(src), "rb").read())
    raw[info["block_offsets"][damaged_block(info) + 1] - 8] ^= 0x10
    with open(str(dst), "wb") as f:
        f.write(bytes(raw))
    shutil.copy(str(src) + ".bai", str(dst) + ".bai")


def sites_args(group):
    s = case()["sites"][group]
    return [x[0] for x in s], [x[1] for x in s], [x[2] for x in s]


def assert_matches_restatement(res, group, K, info):
    """a phase_reads result on write()'s file against expected(group, K): the reads by virtual offset, then array for array"""
    e = expected(group, K)
    got = pu.shaped(res, K)
    assert got["voff"] == [info["voff"][i] for i in e["entered"]]
    for k in ("obs", "link", "phase", "ps", "tags"):
        assert got[k] == e[k], (group, K, k)
    return got


def assert_by_hand(got, group, K, info):
    """the planted facts written out by hand (HAND_OBS, HAND_TAGS), for the groups that hold their reads"""
    names = [info["name_of"][v] for v in got["voff"]]
    if group in ("ops", "all"):
        for name, by_hand in HAND_OBS.items():
            assert got["obs"][names.index(name)] == [(site_index(group, s), x) for s, x in by_hand], name
    if group in ("blocks", "all"):
        for name in HAND_TAGS:
            if K >= 4 or name not in ("only_unphased", "both_sides"):
                assert got["tags"][names.index(name)] == hand_tag(name), (K, name)


def min_cut_chunks(group):
    """the least number of chunks a cut run has to have.  `geom`: with its N_SPARSE sites outside the adjacent run each a chunk's end, an
    uncut run would still give 1 + N_SPARSE chunks; one more than that is a cut inside the run, through the reads that lie over it"""
    return max(MIN_CUT_CHUNKS, 2 + N_SPARSE) if group == "geom" else MIN_CUT_CHUNKS


def small_ends():
    """site lists at the small ends: one site; three sites between two islands, whose reads the chunk's byte range holds and none of
    which enters; three sites behind the last read of q1"""
    gap = island_start(60) + 180
    return {"one_site": [(5100, "A", "C")], "between_islands": [(gap, "A", "C"), (gap + 20, "A", "C"), (gap + 40, "A", "C")],
            "behind_the_reads": [(29000, "A", "C"), (29100, "A", "C"), (29200, "A", "C")]}
