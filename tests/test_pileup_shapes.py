"""The host reader (cto_pack_from_bam, the specification of csrc/pileup.hip) at the shapes of tests/pileuputil.py: long reads of
hundreds to tens of thousands of CIGAR operations, columns of up to 2049 reads, up to 65 indel keys in a column, one to nine accepted
reads.  Every builder case against the naive pile-up of tests/bamutil.py, exactly as test_pack_from_bam_matches_naive_pileup does;
tests/test_gpu_pileup_shapes.py then holds the device to the host reader on the same cases."""
import numpy as np
import pytest

import pileuputil as pu


@pytest.fixture(scope="module")
def bams(tmp_path_factory):
    return pu.Bams(tmp_path_factory.mktemp("pileup_shapes"))


STACKS = pu.STACK_DEPTHS + (200, 2049)
CASES = pu.on_device_cases()
CASES += [("keys65", 0, "keys65"), ("stack2049", 0, "stack2049"), ("stack2049", 1, "stack2049-behind_P"), ("stack200cap199", 0, "stack200cap199")]
CASES += [("stack%dcap%d" % (D, cap), 0, "stack%dcap%d" % (D, cap)) for D in STACKS for cap in (D, D - 1) if (D, cap) not in ((200, 200), (200, 199))]


@pytest.mark.parametrize("name,region_i", [c[:2] for c in CASES], ids=[c[2] for c in CASES])
def test_host_reader_equals_the_naive_pileup(bams, name, region_i):
    c = pu.case(name)
    region = c.regions[region_i]
    got = pu.host_pack(bams(name), c, region)
    pu.assert_same(got, pu.naive_pack(c, region), name)
    pu.assert_reach(name, region_i, got)
    if name.startswith("stack") and region_i == 1:    # no column of D reads, D - 1 reads open at the last read's start all the same
        assert pu.depth_at(got, c.figs["P"]) == 0 and 0 < np.diff(got["col_off"]).max() < c.figs["D"]
    elif name.startswith("stack"):                    # --max-depth on both sides of D: the last read has D - 1 open at its start
        D, cap = c.figs["D"], region[4]
        assert np.diff(got["col_off"]).max() == pu.depth_at(got, c.figs["P"]) == (D if cap >= D else D - 1)
        assert (np.diff(got["key_off"]) > 0).sum() >= 1


def test_cut_independence_of_the_host_reader(bams):
    """the columns of a sub-region are the same whether the whole contig or the sub-region alone is piled up"""
    c = pu.case("long_reads")
    whole, part = pu.host_pack(bams("long_reads"), c, c.regions[0]), pu.host_pack(bams("long_reads"), c, c.regions[4])
    pu.assert_same(pu.restrict(whole, part["col_pos"]), part, "cut")
