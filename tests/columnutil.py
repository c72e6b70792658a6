"""Pileup columns of a chosen composition, for the tests of deep and key-rich columns (test_deep_columns.py, test_gpu_deep_columns.py).

A column is written as a list of runs `(code, kind, bq, mq, key, count)`: `count` consecutive read-bases with base code `code` (an index
into "ACGTacgt*#Nn", or the character), indel kind 0 / 1 (insertion) / 2 (deletion), phred qualities and, for an indel, key = (length,
variant): the inserted sequence is "ACGT"[(variant + i) % 4] for i < length, as the generator writes it, so variant is 0..3.
`run_chunk` turns columns into a SynthChunk-shaped object - the pack arrays plus what the text writers (synth.mpileup_text,
oracle.synth_mpileup_text) read - and `expected_tensor` counts the 34 channels straight from the run lists, in int64 and without any
packed counter, after create_tensor_pileup_calling.py:146-228 of the reference."""
import numpy as np

from clairs_to_amd.synth import BASE_CHARS, SynthChunk

NPOS, NCH, FLANK = 33, 34, 16
A, C, G, T, a, c, g, t, STAR, HASH = range(10)
FWD_CODES = (0, 1, 2, 3, 8, 10)


def _code(x):
    return BASE_CHARS.index(x) if isinstance(x, str) else int(x)


def run_chunk(columns, sites, max_indel_length=60):
    """columns: [(position, reference character, runs)] in increasing position order; sites: the candidate positions."""
    ch = SynthChunk.__new__(SynthChunk)
    ch.max_indel_length = max_indel_length
    ch.site_pos = np.asarray(sorted(sites), dtype=np.int32)
    ch.n_sites = ch.site_pos.size
    ch.col_pos = np.asarray([p for p, _, _ in columns], dtype=np.int32)
    assert (np.diff(ch.col_pos) > 0).all()
    n_cols = ch.col_pos.size
    ch.col_ref_char = np.frombuffer("".join(r for _, r, _ in columns).encode(), dtype=np.uint8).copy()
    idx = np.array(["ACGT".find(chr(r)) for r in ch.col_ref_char.tolist()])
    ch.col_ref = np.where(idx < 0, 0x80, idx).astype(np.uint8)
    rows = np.array([(_code(r[0]), r[1], r[2], r[3], r[4][0] if r[1] else 1, r[4][1] if r[1] else 0, r[5])
                     for _, _, runs in columns for r in runs], dtype=np.int64).reshape(-1, 7)
    assert ((rows[:, 0] >= 0) & (rows[:, 0] < 12) & (rows[:, 1] >= 0) & (rows[:, 1] < 3) & (rows[:, 2] >= 0) & (rows[:, 2] < 94) &
            (rows[:, 3] >= 0) & (rows[:, 3] < 94) & (rows[:, 4] >= 1) & (rows[:, 5] >= 0) & (rows[:, 5] < 4) & (rows[:, 6] >= 0)).all()
    code, okind, bq, mq, ilen, ivar = (np.repeat(rows[:, j], rows[:, 6]) for j in range(6))
    depth = np.array([sum(r[5] for r in runs) for _, _, runs in columns], dtype=np.int64)
    ch.col_off = np.concatenate([[0], np.cumsum(depth)]).astype(np.int64)
    col_of = np.repeat(np.arange(n_cols, dtype=np.int64), depth)
    ch._okind = okind.astype(np.uint8)
    gate = np.where(okind == 1, ilen, ilen + 1)
    kind = np.where((okind > 0) & (gate > max_indel_length), 3, okind).astype(np.uint32)
    kid = ch._index_keys(col_of, code.astype(np.uint32), ilen, ivar, n_cols)
    ch.entries = (code.astype(np.uint32) | (kind << 4) | (bq.astype(np.uint32) << 6) | (mq.astype(np.uint32) << 13) |
                  (kid << 21)).astype(np.uint32)
    ch._ilen = ilen.astype(np.int32)
    ch._ivar = ivar.astype(np.int32)
    return ch


def ref_char(pos):
    """the reference base these tests give a position"""
    return "ACGT"[pos % 4]


def window(pos, centre_runs, neighbour_runs=None, centre_ref=None):
    """The 33 columns pos-16 .. pos+16 with `centre_runs` at the candidate and `neighbour_runs(p)` (default: four forward reference
    bases) elsewhere, as a chunk with the one site `pos`."""
    cols = []
    for p in range(pos - FLANK, pos + FLANK + 1):
        r = ref_char(p)
        if p == pos:
            cols.append((p, centre_ref or r, centre_runs))
        else:
            cols.append((p, r, neighbour_runs(p) if neighbour_runs else [(r, 0, 40, 60, None, 4)]))
    return cols


def column_vector(ref, runs, min_bq, max_indel_length=60):
    """-> (the 34 channels of one column in int64, its depth, {(code, kind, key): count} of the indel keys that count) for the pass
    that sees read-bases with BQ >= min_bq."""
    v = np.zeros(NCH, dtype=np.int64)
    depth = 0
    keys = {}
    for code, kind, bq, mq, key, count in runs:
        code = _code(code)
        if bq < min_bq:
            continue
        if kind == 0:
            if mq >= 20:
                if code < 8:
                    v[code if code < 4 else code + 5] += count
                    depth += count
                elif code in (STAR, HASH):
                    v[8 if code == STAR else 17] += count
                    depth += count
            elif code < 8:
                v[18 + code] += count
            if code < 8 and bq < 30:
                v[26 + code] += count
        elif mq >= 20 and (key[0] if kind == 1 else key[0] + 1) <= max_indel_length:
            fwd = code in FWD_CODES
            v[(4 if kind == 1 else 6) + (0 if fwd else 9)] += count
            depth += count
            k = (code, kind, (key[0], key[1] if kind == 1 else 0))
            keys[k] = keys.get(k, 0) + count
    for (code, kind, _), n in keys.items():
        chn = (5 if kind == 1 else 7) + (0 if code in FWD_CODES else 9)
        v[chn] = max(v[chn], n)
    ri = max("ACGT".find(ref.upper()), 0)          # evc_base_from: anything but ACGT reads as A
    for g0 in (0, 9, 18, 22, 26, 30):
        v[g0 + ri] = -v[g0:g0 + 4].sum()
    return v, depth, keys


def expected_tensor(columns, sites, min_bq, max_indel_length=60):
    """-> (tensor int64 [n, 33, 34], depth int64 [n]) of create_tensor for sites that all have a column and a whole window."""
    vec = {p: column_vector(r, runs, min_bq, max_indel_length) for p, r, runs in columns}
    out = np.zeros((len(sites), NPOS, NCH), dtype=np.int64)
    depth = np.zeros(len(sites), dtype=np.int64)
    for i, s in enumerate(sites):
        assert s in vec and s - FLANK >= 1
        depth[i] = vec[s][1]
        for j in range(NPOS):
            if s - FLANK + j in vec:
                out[i, j] = vec[s - FLANK + j][0]
    return out, depth


def expected_keys(runs, min_bq):
    """Per distinct indel key of one column, in first-seen (= key id) order: [AFF count, NEG count, AFF first index, NEG first index]
    over the read-bases with MQ >= 20 whose indel is not over-long; 0x7fffffff where a pass never meets the key.  Over-long indels
    keep their key id and count nothing."""
    none = 0x7fffffff
    order, at = {}, 0
    for code, kind, bq, mq, key, count in runs:
        if kind:
            k = (_code(code), kind, (key[0], key[1] if kind == 1 else 0))
            rec = order.setdefault(k, [0, 0, none, none])
            if mq >= 20 and (key[0] if kind == 1 else key[0] + 1) <= 60:
                rec[1] += count
                rec[3] = min(rec[3], at)
                if bq >= min_bq:
                    rec[0] += count
                    rec[2] = min(rec[2], at)
        at += count
    return np.array(list(order.values()), dtype=np.int64).reshape(-1, 4)


# ---- the windows the deep-column tests share ------------------------------------------------------------------------------------
LIMIT = 32767            # kMaxDepth of csrc/pack_internal.h
MAX_KEYS = 2048          # kMaxKeysPerCol
POS = 5000               # the candidate of the single-window cases; its reference base is ref_char(POS) = 'A'


def composition_cases():
    """{name: (runs of the 32 767-deep candidate column, {pass: {channel: value}} - every channel of that column that is not zero,
    depth per pass)} with pass 0 = the AFF pass at --min_bq 20, pass 1 = the NEG pass.  The reference base is A."""
    n = LIMIT
    ins = (2, 1)         # the insertion "CG"
    return {
        "fwd_ref": ([(A, 0, 40, 60, None, n)], {0: {0: -n}, 1: {0: -n}}, (n, n)),
        "fwd_alt": ([(C, 0, 40, 60, None, n)], {0: {0: -n, 1: n}, 1: {0: -n, 1: n}}, (n, n)),
        "rev_alt": ([(c, 0, 40, 60, None, n)], {0: {9: -n, 10: n}, 1: {9: -n, 10: n}}, (n, n)),
        "low_bq": ([(C, 0, 10, 60, None, n)], {0: {}, 1: {0: -n, 1: n, 26: -n, 27: n}}, (0, n)),
        "low_mq": ([(C, 0, 40, 19, None, n)], {0: {18: -n, 19: n}, 1: {18: -n, 19: n}}, (0, 0)),
        "one_insertion": ([(A, 1, 40, 60, ins, n)], {0: {4: n, 5: n}, 1: {4: n, 5: n}}, (n, n)),
        "star": ([(STAR, 0, 40, 60, None, n)], {0: {8: n}, 1: {8: n}}, (n, n)),
        "split": ([(C, 0, 40, 60, None, 16384), (G, 0, 40, 60, None, 16383)], {0: {0: -n, 1: 16384, 2: 16383}, 1: {0: -n, 1: 16384, 2: 16383}},
                  (n, n)),
    }


def key_pool():
    """more than MAX_KEYS distinct indel keys (code, kind, key): insertions and deletions on both strands, a few of them over-long"""
    pool = [(code, 1, (ln, var)) for ln in range(1, 64) for var in range(4) for code in range(8)]
    pool += [(code, 2, (ln, 0)) for ln in range(1, 64) for code in range(8)]
    return pool


def key_edge_runs(n_keys, depth=4096, seed=11):
    """One column of `depth` read-bases with exactly n_keys distinct indel keys.  The keys' first occurrences are spread over the whole
    column, the other read-bases are plain bases or repeat a key already met, and qualities vary per read-base: some keys are first
    met on a read-base below --min_bq 20 (the two passes see them first at different indices, or the AFF pass never), some on one
    with MQ < 20 (which counts nowhere)."""
    rng = np.random.default_rng(seed + n_keys)
    pool = key_pool()
    keys = [pool[i] for i in rng.permutation(len(pool))[:n_keys]]
    first_at = np.sort(rng.choice(depth, size=n_keys, replace=False))
    first_at[-1] = max(first_at[-1], depth - 3)            # one key is first met in the column's last read-bases
    assert np.unique(first_at).size == n_keys
    is_first = np.zeros(depth, dtype=bool)
    is_first[first_at] = True
    runs, seen = [], 0
    for i in range(depth):
        bq = int(rng.choice((10, 25, 40), p=(0.3, 0.2, 0.5)))
        mq = 60 if rng.random() < 0.85 else 10
        if is_first[i]:
            code, kind, key = keys[seen]
            seen += 1
        elif seen and rng.random() < 0.5:
            code, kind, key = keys[int(rng.integers(0, seen))]
        else:
            code, kind, key = int(rng.integers(0, 10)), 0, None
        runs.append((code, kind, bq, mq, key, 1))
    assert seen == n_keys
    return runs


def gate_columns():
    """Columns that sit exactly on candidate extraction's gates (reference base A, every read-base BQ 40 / MQ 60), with the parameter
    sets they are meant for: -> (columns, [(params, {position: (SNV candidate, indel candidate)})]).  params = (snv_min_af, indel_min_af,
    min_coverage, alt_base_num); a position a set does not list is not asserted by hand for it (the oracle still is, for all)."""
    def snv(depth, alt):
        return [(A, 0, 40, 60, None, depth - alt), (C, 0, 40, 60, None, alt)]

    def alleles(big):
        # 20 distinct merged insertion alleles: 19 of 100 read-bases and one of `big`, among forward reference bases
        runs = [(A, 1, 40, 60, (3 + k // 4, k % 4), 100) for k in range(19)]
        runs += [(A, 1, 40, 60, (9, 0), big), (A, 0, 40, 60, None, LIMIT - 1900 - big)]
        return runs

    p = 8000                                              # p % 4 == 0: the reference base of every column below is A
    cols = [(p, "A", snv(32760, 1638)),                   # AF = 0.05 exactly: passes
            (p + 4, "A", snv(32760, 1637)),               # just below
            (p + 8, "A", snv(40, 3)),                     # alt_base_num = 3 met exactly
            (p + 12, "A", snv(40, 2)),                    # AF = 0.05, but two read-bases
            (p + 16, "A", snv(4, 3)),                     # depth == min_coverage: `>` fails
            (p + 20, "A", snv(5, 3)),                     # min_coverage + 1
            (p + 24, "A", snv(32761, 1639)),
            (p + 28, "A", alleles(1639)),                 # 1639 / 32767 >= 0.05
            (p + 32, "A", alleles(1638))]                 # 1638 / 32767 <  0.05
    want = [((0.05, 0.05, 4, 3), {p: (1, 0), p + 4: (0, 0), p + 8: (1, 0), p + 12: (0, 0), p + 16: (0, 0), p + 20: (1, 0), p + 24: (1, 0),
                                  p + 28: (0, 1), p + 32: (0, 0)}),
            ((0.01, 0.01, 4, 1638), {p: (1, 0), p + 4: (0, 0), p + 24: (1, 0), p + 28: (0, 1), p + 32: (0, 1)}),     # the count gate at depth
            ((0.05, 0.05, 32760, 3), {p: (0, 0), p + 24: (1, 0), p + 28: (0, 1)})]                              # the coverage gate at depth
    return cols, want
