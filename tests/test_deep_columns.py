"""The host side of the column limits (csrc/pack_internal.h: 32 767 read-bases and 2 048 distinct indel keys per column) and the
inputs of test_gpu_deep_columns.py: one past a limit is CTO_EUNSUPPORTED on every host constructor, the generator's new depth
arguments leave its default chunks as they were, and the oracle's tensors of the composition-controlled columns are what a plain
count over their run lists gives.  No GPU."""
import hashlib

import numpy as np
import pytest

import columnutil as cu

REF = "ACGT" * 50
QUAL = "I"          # phred 40
MAPQ = "]"          # phred 60


def _row(pos, tokens):
    n = len(tokens)
    return "chr1\t%d\tN\t%d\t%s\t%s\t%s\n" % (pos, n, "".join(tokens), QUAL * n, MAPQ * n)


def _one_column(depth, n_keys):
    """pack arrays of one column: n_keys read-bases that each carry an insertion key of their own, then plain bases"""
    ent = np.full(depth, 0 | (40 << 6) | (60 << 13), dtype=np.uint32)
    ent[:n_keys] |= (1 << 4) | (np.arange(n_keys, dtype=np.uint32) << 21)
    return dict(col_pos=np.array([40], dtype=np.int32), col_ref=np.array([3], dtype=np.uint8), col_off=np.array([0, depth], dtype=np.int64),
                key_off=np.array([0, n_keys], dtype=np.int32), entries=ent, key_meta=np.full(n_keys, 1 | 4, dtype=np.uint8),
                key_group=np.arange(n_keys, dtype=np.int32))


def _insertion(i):
    return "A+6" + "".join("ACGT"[(i >> (2 * j)) & 3] for j in range(6))


def _unsupported(exc):
    return "error -4:" in str(exc.value)         # CTO_EUNSUPPORTED


def test_depth_limit_of_the_text_constructor():
    from clairs_to_amd._lib import CtoError
    from clairs_to_amd.pack import ColumnPack
    pack = ColumnPack.from_mpileup(_row(40, ["A"] * cu.LIMIT), REF, 1)
    assert pack.n_entries == cu.LIMIT and pack.numpy()["col_off"].tolist() == [0, cu.LIMIT]
    with pytest.raises(CtoError) as e:
        ColumnPack.from_mpileup(_row(40, ["A"] * (cu.LIMIT + 1)), REF, 1)
    assert _unsupported(e) and "32768" in str(e.value)
    with pytest.raises(CtoError) as e:                 # a deep row among others
        ColumnPack.from_mpileup(_row(39, ["A"] * 5) + _row(40, ["c"] * (cu.LIMIT + 1)) + _row(41, ["A"] * 5), REF, 1)
    assert _unsupported(e) and "32768" in str(e.value)


def test_depth_limit_of_the_array_constructor():
    from clairs_to_amd._lib import CtoError
    from clairs_to_amd.pack import ColumnPack
    pack = ColumnPack.from_arrays(**_one_column(cu.LIMIT, 0))
    assert pack.n_entries == cu.LIMIT
    with pytest.raises(CtoError) as e:
        ColumnPack.from_arrays(**_one_column(cu.LIMIT + 1, 0))
    assert _unsupported(e) and "32768" in str(e.value)


def test_key_limit_of_the_text_constructor():
    from clairs_to_amd._lib import CtoError
    from clairs_to_amd.pack import ColumnPack
    pack = ColumnPack.from_mpileup(_row(40, [_insertion(i) for i in range(cu.MAX_KEYS)] * 2), REF, 1)
    a = pack.numpy()
    assert pack.n_keys == cu.MAX_KEYS and a["key_off"].tolist() == [0, cu.MAX_KEYS]
    np.testing.assert_array_equal(a["entries"] >> 21, np.tile(np.arange(cu.MAX_KEYS, dtype=np.uint32), 2))     # ids in first-seen order, up to 2 047
    with pytest.raises(CtoError) as e:
        ColumnPack.from_mpileup(_row(40, [_insertion(i) for i in range(cu.MAX_KEYS + 1)]), REF, 1)
    assert _unsupported(e) and "2048" in str(e.value)


def test_key_limits_of_the_array_constructor():
    from clairs_to_amd._lib import CtoError
    from clairs_to_amd.pack import ColumnPack
    pack = ColumnPack.from_arrays(**_one_column(4096, cu.MAX_KEYS))
    assert pack.n_keys == cu.MAX_KEYS
    with pytest.raises(CtoError) as e:
        ColumnPack.from_arrays(**_one_column(4096, cu.MAX_KEYS + 1))
    assert _unsupported(e) and "2049" in str(e.value)
    # an indel entry that names a key its column does not have: CTO_EINVAL, whatever its kind (over-long indels keep a key too)
    for kind in (1, 2, 3):
        arr = _one_column(100, 7)
        arr["entries"][50] = 0 | (kind << 4) | (40 << 6) | (60 << 13) | (7 << 21)
        with pytest.raises(CtoError) as e:
            ColumnPack.from_arrays(**arr)
        assert "error -1:" in str(e.value) and "key 7" in str(e.value)
        arr["entries"][50] = 0 | (kind << 4) | (40 << 6) | (60 << 13) | (6 << 21)
        assert ColumnPack.from_arrays(**arr).n_keys == 7
    # the key id bits of a plain base mean nothing
    arr = _one_column(100, 7)
    arr["entries"][50] |= np.uint32(2047 << 21)
    assert ColumnPack.from_arrays(**arr).n_entries == 100
    # two columns: the second one's ids are checked against its own count
    two = _one_column(100, 7)
    two.update(col_pos=np.array([40, 41], dtype=np.int32), col_ref=np.array([3, 0], dtype=np.uint8), col_off=np.array([0, 60, 100], dtype=np.int64),
               key_off=np.array([0, 7, 7], dtype=np.int32))
    assert ColumnPack.from_arrays(**two).n_cols == 2
    two["entries"][70] |= np.uint32(1 << 4)
    with pytest.raises(CtoError) as e:
        ColumnPack.from_arrays(**two)
    assert "error -1:" in str(e.value)
    for bad in ([0, 8], [7, 0], [-1, 7]):                 # key_off that leaves the key arrays or runs backwards
        arr = _one_column(100, 7)
        arr["key_off"] = np.array(bad, dtype=np.int32)
        with pytest.raises(CtoError) as e:
            ColumnPack.from_arrays(**arr)
        assert "error -1:" in str(e.value)


# sha256 over arrays(), site_pos, _okind, _ilen and _ivar (name, dtype, shape and bytes of each, names sorted), computed with the
# generator as it was before it had `depth_max` and `depth`
PARENT_DIGESTS = {
    "seed20260928": "57d96513eb524627b0309eb80184016d5d0e6417a6738cccdfaa0da6705253ad",
    "ont": "57d96513eb524627b0309eb80184016d5d0e6417a6738cccdfaa0da6705253ad",
    "ilmn": "5d132562f352aac582148a4b5207b962731b11c2f311d9b52401ee20fe32eebe",
    "hifi": "d49ac845f0583ee32dc2da0af60c16c46640c355a70f800f20530c61865819d0",
}


def _digest(ch):
    h = hashlib.sha256()
    arrs = dict(ch.arrays(), site_pos=ch.site_pos, _okind=ch._okind, _ilen=ch._ilen, _ivar=ch._ivar)
    for k in sorted(arrs):
        a = np.ascontiguousarray(arrs[k])
        h.update(("%s:%s:%s;" % (k, a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def test_default_chunks_are_what_they_were():
    from clairs_to_amd.synth import SynthChunk
    assert _digest(SynthChunk(64, seed=20260928)) == PARENT_DIGESTS["seed20260928"]
    for p in ("ont", "ilmn", "hifi"):
        assert _digest(SynthChunk.for_platform(p, 64)) == PARENT_DIGESTS[p], p
    assert _digest(SynthChunk(64, seed=20260928, depth_max=200)) == PARENT_DIGESTS["seed20260928"]


def test_depth_arguments_of_the_generator():
    from clairs_to_amd.synth import SynthChunk
    assert np.diff(SynthChunk(20, seed=3, depth_mean=600.0).col_off).max() == 200
    deep = SynthChunk(20, seed=3, depth_mean=600.0, depth_max=1000)
    assert 400 < np.diff(deep.col_off).max() <= 1000
    flat = SynthChunk(1, seed=3, depth=4097)
    assert flat.col_pos.size == 34 and (np.diff(flat.col_off) == 4097).all()
    per_col = np.arange(34) + 1
    assert (np.diff(SynthChunk(1, seed=3, depth=per_col).col_off) == per_col).all()
    # the clip and the override consume no random numbers: positions and reference bases are the default chunk's
    base = SynthChunk(20, seed=3)
    assert np.array_equal(deep.site_pos, base.site_pos) and np.array_equal(deep.col_ref, base.col_ref)
    with pytest.raises(AssertionError):
        SynthChunk(1, seed=3, depth=cu.LIMIT + 1)


def _window_case(name):
    if name.startswith("keys"):
        return cu.window(cu.POS, cu.key_edge_runs(int(name[4:])))
    return cu.window(cu.POS, cu.composition_cases()[name][0])


@pytest.mark.parametrize("name", list(cu.composition_cases()) + ["keys257", "keys2048"])
def test_oracle_agrees_with_a_count_over_the_run_list(oracle_lib, name):
    """create_tensor of the oracle on the text of a composition-controlled window == the channels counted straight from its runs in
    int64 (columnutil.expected_tensor), for both passes; and the pack the text tokenises to is the arrays the run list was turned
    into.  This pins what test_gpu_deep_columns.py expects of these windows without any kernel."""
    from clairs_to_amd.pack import ColumnPack
    cols = _window_case(name)
    ch = cu.run_chunk(cols, [cu.POS])
    ref, lo = ch.ref_window()
    assert ch.col_pos.size == 33 and ref[cu.POS - lo] == "A"
    for p, q in ((0, 20), (1, 0)):
        text = oracle_lib.synth_mpileup_text(ch, q)
        t, depth, alts, flags = oracle_lib.create_tensor(text, ref, lo, ch.site_pos, alt_stride=1 << 18)
        want, want_depth = cu.expected_tensor(cols, [cu.POS], q)
        np.testing.assert_array_equal(t, want)
        assert depth.tolist() == want_depth.tolist() and flags.tolist() == [0]
        if not name.startswith("keys"):
            _, nonzero, d = cu.composition_cases()[name]
            assert {int(i): int(t[0, 16, i]) for i in np.nonzero(t[0, 16])[0]} == nonzero[p] and depth[0] == d[p]
    pack = ColumnPack.from_mpileup(oracle_lib.synth_mpileup_text(ch, 0), ref, lo)
    got, arr = pack.numpy(), ch.arrays()               # views into `pack`
    for k in arr:
        np.testing.assert_array_equal(got[k], arr[k], err_msg=k)
    if name.startswith("keys"):
        nk = int(name[4:])
        assert arr["key_off"][17] - arr["key_off"][16] == nk and int((arr["entries"] >> 21).max()) == nk - 1
        assert cu.expected_keys(cols[16][2], 20).shape == (nk, 4)


@pytest.mark.parametrize("select_indel", [True, False])
def test_gate_columns_land_on_the_intended_side_in_the_oracle(oracle_lib, select_indel):
    cols, sets = cu.gate_columns()
    ch = cu.run_chunk(cols, [])
    ref, lo = ch.ref_window()
    text6 = oracle_lib.synth_mpileup_text(ch, 20, None, 20, False)
    assert int(np.diff(ch.key_off).max()) == 20 and int(ch.key_group.max()) == 19          # more merged alleles than a lane holds in LDS
    for (snv_af, indel_af, cov, abn), by_hand in sets:
        pos, fl, dep = oracle_lib.extract_candidates(text6, ref, lo, snv_af, indel_af, cov, abn, select_indel)
        assert pos.tolist() == ch.col_pos.tolist() and dep.tolist() == np.diff(ch.col_off).tolist()
        at = {int(p): int(f) for p, f in zip(pos, fl)}
        for p, (snv, indel) in by_hand.items():
            assert (at[p] & 1, (at[p] >> 1) & 1) == (snv, indel if select_indel else 0), (snv_af, cov, abn, p)
