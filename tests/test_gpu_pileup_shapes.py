"""csrc/pileup.hip at the shapes it was written for and at its own limits (builders: tests/pileuputil.py): CIGARs of hundreds to
70 000 operations (k_fill's batches of 64, the look-ahead across a batch boundary), aligned runs around LONG_OP = 48, 64 and 256
positions, 63 .. 2047 reads open at a read's start (every live_cap from 64 to 2048, the 64 KB launch), columns of 2048 and 2049
reads, --max-depth on both sides of the depth, 63 / 64 / 65 indel keys in a column, one to nine accepted reads over the eight XCDs.
The specification is the host reader, which tests/test_pileup_shapes.py holds to the naive pile-up on the same cases: every array
and every key string equal, and no case may pass by falling back."""
import numpy as np
import pytest

import pileuputil as pu
from test_gpu_pileup import _device_arrays

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bams(tmp_path_factory):
    return pu.Bams(tmp_path_factory.mktemp("gpu_pileup_shapes"))


def _pileup(dp, dev, bam, c, region):
    """(device pack as host arrays or None, fallback)"""
    from clairs_to_amd._lib import lib
    ri, start, end, bed, max_depth = region
    pv, lite, fallback = dp.pileup(bam, None, c.refs[ri][0], start, end, c.ref_seqs[ri], 1, dev, bed=bed, min_mq=c.figs.get("min_mq", 0),
                                   max_depth=max_depth)
    if fallback:
        return None, True
    got = _device_arrays(pv, lite)
    lib.cto_pack_free(lite)
    return got, False


def _on_device_equal(dp, dev, bams, name, region_i=0):
    c = pu.case(name)
    region = c.regions[region_i]
    want = pu.host_pack(bams(name), c, region)
    pu.assert_reach(name, region_i, want)
    got, fallback = _pileup(dp, dev, bams(name), c, region)
    assert not fallback, name
    pu.assert_same(got, want, name)
    return got, want


CASES = pu.on_device_cases()


@pytest.mark.parametrize("name,region_i", [c[:2] for c in CASES], ids=[c[2] for c in CASES])
def test_device_pileup_equals_the_host_reader_at(dev, bams, name, region_i):
    from clairs_to_amd.bgzf import DevicePileup
    got, want = _on_device_equal(DevicePileup(), dev, bams, name, region_i)
    f = pu.case(name).figs
    if name.startswith("stack"):
        assert np.diff(got["col_off"]).max() == pu.depth_at(got, f["P"]) == f["D"]
    if name.startswith("keys"):
        assert np.diff(got["key_off"]).max() == f["K"]


@pytest.mark.parametrize("name,region_i", [("stack2049", 0), ("stack2049", 1), ("stack200cap199", 0), ("keys65", 0)],
                         ids=["stack2049", "stack2049-behind_P", "stack200cap199", "keys65"])
def test_device_pileup_falls_back_past_its_limits_and_goes_on(dev, bams, name, region_i):
    """a column of 2049 reads; 2048 reads open at the last read's start where the BED asks for no column deeper than 2048; --max-depth
    reads open at a read's start; a 65th indel key in a column: `fallback`, never a different pack - and the same context piles up
    the next chunk right"""
    from clairs_to_amd.bgzf import DevicePileup
    c = pu.case(name)
    want = pu.host_pack(bams(name), c, c.regions[region_i])
    pu.assert_reach(name, region_i, want)            # what the host reader then gives: tests/test_pileup_shapes.py
    if (name, region_i) == ("stack2049", 1):
        assert 0 < np.diff(want["col_off"]).max() <= 2048
    dp = DevicePileup()
    got, fallback = _pileup(dp, dev, bams(name), c, c.regions[region_i])
    assert fallback and got is None
    _on_device_equal(dp, dev, bams, "stack64")
    _on_device_equal(dp, dev, bams, "keys63")


def test_device_pileup_does_not_depend_on_the_cut(dev, bams):
    """the columns of a sub-region out of the whole contig's pack = the pack of the sub-region piled up alone: an entry's place may
    not depend on what else is in the chunk"""
    from clairs_to_amd.bgzf import DevicePileup
    c = pu.case("long_reads")
    dp = DevicePileup()
    whole, fb_w = _pileup(dp, dev, bams("long_reads"), c, c.regions[0])
    part, fb_p = _pileup(dp, dev, bams("long_reads"), c, c.regions[4])
    assert not fb_w and not fb_p
    assert len(part["col_pos"]) == c.regions[4][2] - c.regions[4][1] + 1
    pu.assert_same(pu.restrict(whole, part["col_pos"]), part, "cut")
