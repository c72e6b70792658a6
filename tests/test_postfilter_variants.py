"""postfilter_variants on the CPU: the parser against the reference's option table and the argv `run_clairs_to --dry_run` builds, the host
packer (cto_postfilter_pack) against hand-written rows for each quirk of get_base_list / _parse_mpileup_postfilter_chunk_dict, the Python
restatements of Fisher's test and the sequence entropy against values recorded from the reference, and the fixture itself: inputs pinned by
SHA-256, the coverage the generator asserted re-asserted from the stored outputs (tests/golden/postfilter.json.gz, gen_postfilter.py)."""
import pytest

from conftest import load_json_gz
from test_cli_argv import SAMPLE, fill

TAGS = ("ReadStartEnd", "VariantCluster", "StrandBias", "LowSeqEntropy")
SUPERSEDED, RSE, ENDS0, ENDS1, EXTRA, TOKEN = 0x80000000, 0x40000000, 0x20000000, 0x10000000, 0x08000000, 0xfffff


@pytest.fixture(scope="module")
def golden():
    return load_json_gz("postfilter.json.gz")


def parser():
    from clairs_to_amd.postfilter_variants import build_parser
    return build_parser()


def test_is_a_submodule():
    from clairs_to_amd.__main__ import SUBMODULES
    assert "postfilter_variants" in SUBMODULES


def test_every_reference_option_is_accepted(golden):
    table = golden["parser"]
    assert len(table) >= 30
    everything = []
    for opt in table:
        name = opt["options"][-1]
        argv = [name] if opt["action"] == "_StoreTrueAction" else [name, SAMPLE[opt["type"]]]
        parser().parse_args(argv)
        everything += argv
    a = parser().parse_args(everything)
    assert a.flanking == 7 and a.is_indel and a.enable_postfilter is True and a.input_filter_tag is None and a.pos == 7


def test_the_dry_run_argv_parses(golden):
    seen = set()
    for inv in golden["argv"]:
        a = parser().parse_args(fill(inv["argv"], inv["source"]))
        assert a.pileup_vcf_fn.endswith("_pileup_realignment.vcf") and a.output_dir.endswith("/vcf_output") and a.pos is None
        seen.add(a.is_indel)
    assert seen == {True, False}


# ------------------------------------------------------------------------------------------ the packer
def pack(rows, ref="ACGTACGTAC", lo=1, flanking=100):
    from clairs_to_amd.postfilter_variants import PackedJob
    return PackedJob("".join(rows), ref, lo, flanking).view()


def column(v, c):
    a, b = int(v["col_off"][c]), int(v["col_off"][c + 1])
    return [(int(t), v["keys"][int(r)]) for t, r in zip(v["ent_tok"][a:b], v["ent_rid"][a:b])]


def row(pos, bases, names, more=""):
    n = len(names.split(","))
    return "chr1\t%d\tN\t%d\t%s\t%s\t%s\t%s%s\n" % (pos, n, bases, "I" * n, "]" * n, names, more)


def test_packer_keys_tokens_and_strands():
    v = pack([row(2, "Ac+2tg*#-1nG", "r1,r2,r3,r4,r5", "\textra")])
    assert v["col_pos"].tolist() == [2]
    assert v["tokens"] == [["A", "C+TG", "*", "#-N", "G"]]                            # the indel string drops its length digits (:166)
    ent = column(v, 0)
    assert [k for _, k in ent] == ["r1_0", "r2_1", "r3_0", "r4_1", "r5_0"]          # lower case and '#' are the reverse strand
    assert [t & TOKEN for t, _ in ent] == [0, 1, 2, 3, 4]
    assert [bool(t & ENDS0) for t, _ in ent] == [True, False, True, False, True] and [bool(t & ENDS1) for t, _ in ent] == [False, True, False, True, False]
    meta = v["tok_meta"].tolist()
    assert [m & 3 for m in meta] == [0, 0, 2, 0, 0]                                  # ref base at POS 2 is C; '*' is flagged, '#-N' is not
    assert [m >> 8 for m in meta] == [0, 0, 0, 0, 0]                                 # "+tg" is not longer than 3
    assert v["tok_cnt"].tolist() == [1, 1, 1, 1, 1]


def test_packer_reference_base_and_insertion_share():
    v = pack([row(3, "GGg+4acgtG+300" + "A" * 300, "a,b,c,d")], flanking=100)
    assert v["tokens"] == [["G", "G+ACGT", "G+" + "A" * 300]]
    assert [m & 1 for m in v["tok_meta"].tolist()] == [1, 0, 0]
    assert [m >> 8 for m in v["tok_meta"].tolist()] == [0, 4, 200]                   # min(len - 1, 2 * flanking)
    assert v["tok_cnt"].tolist() == [2, 1, 1]
    assert pack([row(3, "G+300" + "A" * 300, "a")], flanking=50)["tok_meta"].tolist()[0] >> 8 == 100


def test_packer_caret_marks_the_entry_before_it():
    # '^' at the start of the row -> index -1 = the row's LAST name; two starts beat one end
    v = pack([row(1, "^]AC^]G$T", "a,b,c,d")])
    assert [bool(t & RSE) for t, _ in column(v, 0)] == [False, True, False, True]
    assert v["col_flags"].tolist() == [1]                                            # 2 >= 4 * 0.2
    # a tie keeps the END set: '$' marks the current entry
    v = pack([row(1, "A^]C$GT", "a,b,c,d")])
    assert [bool(t & RSE) for t, _ in column(v, 0)] == [False, True, False, False]
    # the character after '^' is skipped even when it is a base or '$'
    v = pack([row(1, "A^$C^AG", "a,b,c")])
    assert v["tokens"] == [["A", "C", "G"]] and [bool(t & RSE) for t, _ in column(v, 0)] == [True, True, False]


def test_packer_start_end_threshold():
    # len(set) >= len(entries) * 0.2 (:409): 2 of 10 qualify, 1 of 10 does not, 1 of 3 does (1 >= 0.6000000000000001)
    names = ",".join("r%d" % i for i in range(10))
    v = pack([row(1, "C$C$" + "C" * 8, names), row(2, "C$" + "C" * 9, names), row(3, "C$CC", "a,b,c")])
    assert v["col_flags"].tolist() == [1, 0, 1]


def test_packer_other_characters_short_rows_and_last_name():
    rows = ["chr1\t1\tN\t2\tAC\tII\t]]\n",                                           # seven fields: skipped
            "chr1\t2\tN\t3\tA>.,<c\tIII\t]]]\tx,y,z\n"]                              # '>' '.' ',' '<' make no entry: two entries, three names
    v = pack(rows)
    assert v["col_pos"].tolist() == [2] and v["tokens"] == [["A", "C"]]
    ent = column(v, 0)
    assert [k for _, k in ent] == ["x_0", "y_1", "z\n"]                              # the 8th field ends the row: its last name keeps the '\n'
    assert bool(ent[2][0] & EXTRA) and not ent[2][0] & (ENDS0 | ENDS1)
    # with a ninth field the last name is clean, and it is the same key as elsewhere
    v = pack([row(1, "AC", "x,y"), row(2, "AC", "y,x", "\t1,2")])
    assert [k for _, k in column(v, 0)] == ["x_0", "y\n_0"] and [k for _, k in column(v, 1)] == ["y_0", "x_0"]
    assert v["keys"] == ["x_0", "y\n_0", "y_0"]                                      # interned per job, first seen first


def test_packer_repeated_keys_and_per_column_tokens():
    v = pack([row(1, "ATAg", "p,q,p,p", "\t-"), row(2, "TTA", "p,q,r", "\t-")])
    ent = column(v, 0)
    assert [k for _, k in ent] == ["p_0", "q_0", "p_0", "p_1"]
    assert [bool(t & SUPERSEDED) for t, _ in ent] == [True, False, False, False]     # dict(zip()) keeps the last p_0
    assert v["tokens"] == [["A", "T", "G"], ["T", "A"]] and v["tok_cnt"].tolist() == [2, 1, 1, 2, 1]          # the counter counts every entry
    assert [t & TOKEN for t, _ in column(v, 1)] == [0, 0, 1]


def test_packer_rejects_what_the_reference_raises_on():
    from clairs_to_amd._lib import CtoError
    with pytest.raises(CtoError):
        pack([row(1, "ACG", "a,b")])                                                 # more entries than names
    with pytest.raises(CtoError):
        pack([row(5, "A", "a"), row(4, "A", "a")])


# ------------------------------------------------------------------------------------------ host scalars
def test_fisher_is_the_references(golden):
    from clairs_to_amd.postfilter_variants import fisher_exact_two_sided
    assert len(golden["fisher"]) >= 60
    for rec in golden["fisher"]:
        p = fisher_exact_two_sided(*rec["table"])
        assert repr(p) == rec["p"] and str(round(p, 5)) == rec["rounded"], rec
    assert any("e" in r["rounded"] for r in golden["fisher"])


def test_entropy_is_the_references(golden):
    from clairs_to_amd.postfilter_variants import sequence_entropy
    assert len(golden["entropy"]) >= 20
    for rec in golden["entropy"]:
        assert repr(sequence_entropy(rec["seq"])) == rec["value"], rec
    vals = [float(r["value"]) for r in golden["entropy"]]
    assert min(vals) < 0.9 < max(vals)


# ------------------------------------------------------------------------------------------ the fixture
def evaluated(golden):
    out = []
    for sc in golden["scenarios"]:
        for run in sc["runs"]:
            for r in (run["out_vcf"] or "").split("\n"):
                c = r.split("\t")
                if len(c) > 7 and r[0] != "#" and ";SB=" in c[7]:
                    out.append((set(c[6].split(";")) & set(TAGS), c[7].rsplit(";SB=", 1)[1]))
    return out


def test_fixture_inputs_are_pinned(golden):
    import pfsim
    for sc in golden["scenarios"]:
        assert pfsim.digest(pfsim.scenario_files(sc["spec"])) == sc["inputs_sha256"], sc["name"]


def test_fixture_coverage(golden):
    ev = evaluated(golden)
    assert len(ev) >= 300
    for tag in TAGS:
        n = sum(tag in t for t, _ in ev)
        assert n >= 10 and len(ev) - n >= 10, tag
    assert sum(len(t) >= 2 for t, _ in ev) >= 5
    assert any("e" in sb for _, sb in ev) and any("e" not in sb for _, sb in ev)
    for sc in golden["scenarios"]:
        for run in sc["runs"]:
            assert run["same_in_both_modes"] in (None, True), run["name"]
    names = {r["name"] for sc in golden["scenarios"] for r in sc["runs"]}
    assert {"chr1_snv", "chr1_indel", "no_ctg_snv", "show_ref", "filter_tag", "no_rse", "cov3", "flank50", "off", "test_pos", "odd_snv", "odd_indel"} <= names
    assert sum(len(sc["per_pos"]) for sc in golden["scenarios"]) >= 10
