"""The BGZF coder on the device (csrc/deflate.hip) against its host restatement (csrc/deflate_host.h): the same bytes for every shape
of tests/bgzfdeflateutil.py, the same counts, through both test seams, on a stream of its own, and in the two writers that use it.  What
the host restatement itself is held to: tests/test_bgzf_deflate.py."""
import ctypes as C

import numpy as np
import pytest

import bamutil
import contamutil as cu
import bgzfdeflateutil as du
import phaseutil as pu

pytestmark = pytest.mark.gpu

SHAPES = du.shapes()
COUNTS = ("n_blocks", "in_bytes", "out_bytes", "stored", "fixed", "dynamic")


def read(fn):
    with open(fn, "rb") as f:
        return f.read()


def both(raw, **kw):
    from clairs_to_amd import bgzf
    from clairs_to_amd._lib import DeflateStats
    st_h, st_d = DeflateStats(), DeflateStats()
    host = bgzf.deflate_blocks(raw, where="host", stats=st_h)
    dev = bgzf.deflate_blocks(raw, where="device", stats=st_d, **kw)
    return host, dev, st_h, st_d


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_device_bytes_equal_host_bytes(name):
    import torch
    from clairs_to_amd import bgzf
    raw = SHAPES[name]
    (hb, hs), (db, ds), st_h, st_d = both(raw)
    assert db == hb and list(ds) == list(hs)
    for f in COUNTS:
        assert getattr(st_d, f) == getattr(st_h, f), f
    assert st_h.n_blocks == (len(raw) + du.PAYLOAD - 1) // du.PAYLOAD and st_h.in_bytes == len(raw) and st_h.out_bytes == len(hb)
    du.check_blocks(raw, db, ds)
    assert b"".join(bgzf.inflate_bytes(db + du.EOF_BLOCK, torch.device("cuda:0"))) == raw          # the package's own decoder, on the device


def test_three_blocks_on_a_stream_of_its_own():
    import torch
    raw = du.bam_like(2 * du.PAYLOAD + 999, 21)
    s = torch.cuda.Stream()
    (hb, hs), (db, ds), _, st_d = both(raw, stream=s)
    assert db == hb and list(ds) == list(hs) and st_d.n_blocks == 3 and st_d.ms_kernels > 0


def test_code_length_seam():
    cases = {"fibonacci22_of_286": (du.fibonacci_freq(22, 286, stride=13), 15), "fibonacci19": (du.fibonacci_freq(19, 19), 7),
             "one": ([0] * 200 + [3] + [0] * 85, 15), "none": ([0] * 30, 15), "two": ([0, 0, 0, 7, 0, 1] + [0] * 24, 15),
             "equal286": ([3] * 286, 15), "equal19": ([1] * 19, 7), "skewed": ([1 + (k * k) % 97 + (40000 if k == 101 else 0) for k in range(286)], 15),
             "ties": ([k % 4 for k in range(288)], 15)}
    for name, (freq, max_bits) in cases.items():
        assert du.code_lengths(freq, max_bits, "device") == du.code_lengths(freq, max_bits, "host"), name


@pytest.mark.parametrize("name", ["n1", "n4", "payload", "equal", "random", "crafted", "no_match", "segment_end", "all_bytes"])
def test_block_size_seam(name):
    block = SHAPES[name][:du.PAYLOAD]
    bits_h, hist_h = du.block_sizes(block, "host")
    bits_d, hist_d = du.block_sizes(block, "device")
    assert bits_d == bits_h and list(hist_d) == list(hist_h)


@pytest.fixture(scope="module")
def bams(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_deflate")
    out = {"dir": d}
    sims = {s: pu.sim_case(s) for s in (7, 11)}
    for level in (0, 6):
        t, n = str(d / ("t_l%d.bam" % level)), str(d / ("n_l%d.bam" % level))
        bamutil.write_bam(t, cu.HAND_REFS, cu.mix_reads("t"), block_payload=3000, level=level)
        bamutil.write_bam(n, cu.HAND_REFS, cu.mix_reads("n"), block_payload=3000, level=level)
        out["hand", level] = dict(t=t, n=n)
        st, sn = str(d / ("sim7_l%d.bam" % level)), str(d / ("sim11_l%d.bam" % level))
        refs = [(pu.SIM_CTG, sims[7]["ref_len"])]
        bamutil.write_bam(st, refs, sims[7]["reads"], level=level)
        bamutil.write_bam(sn, refs, [dict(r, name="n" + r["name"]) for r in sims[11]["reads"]], level=level)
        out["sim", level] = dict(t=st, n=sn)
    return out


@pytest.mark.parametrize("level", [0, 6])
@pytest.mark.parametrize("which", ["hand", "sim"])
def test_mix_device_coder_equals_host_coder(bams, which, level, monkeypatch):
    from clairs_to_amd.gen_contaminated_bam import mix_bams
    monkeypatch.setenv("CTO_CONTAM_CHUNK_BYTES", "20000")                      # hand: several windows, bytes carried on the device
    b, d = bams[which, level], bams["dir"]
    outs, stats, dstats = {}, {}, {}
    for tag, where, deflate in (("hh", "host", "host"), ("dd", "device", "device"), ("hd", "host", "device"), ("dh", "device", "host")):
        outs[tag], stats[tag], dstats[tag] = str(d / ("%s%d_%s.bam" % (which, level, tag))), {}, {}
        mix_bams(b["t"], b["n"], outs[tag], 600, 400, seed=2, where=where, host_threads=2, stats=stats[tag], deflate=deflate, deflate_stats=dstats[tag])
    assert stats["dd"]["fallback_chunks"] == 0 and stats["dh"]["fallback_chunks"] == 0
    assert stats["dd"]["n_chunks"] == stats["hh"]["n_chunks"] >= (4 if which == "hand" else 1)
    for tag in ("dd", "hd", "dh"):
        assert read(outs[tag]) == read(outs["hh"]) and read(outs[tag] + ".bai") == read(outs["hh"] + ".bai"), tag
        for f in COUNTS:
            assert dstats[tag][f] == dstats["hh"][f], (tag, f)
    assert dstats["dd"]["ms_kernels"] > 0 and dstats["dd"]["n_blocks"] == len(cu.block_sizes(outs["dd"])) - 1
    stream, eof = cu.inflated(outs["dd"])
    assert eof and len(stream) == stats["dd"]["out_bytes"]


def test_phase_tumor_device_coder_equals_host_coder(tmp_path, monkeypatch):
    from test_bgzf_deflate import phase_cli, phase_inputs
    from clairs_to_amd import phase_tumor as pt
    phase_inputs(tmp_path)
    monkeypatch.setattr(pt.BatchBgzfWriter, "BATCH", 3)
    host, dev = phase_cli(tmp_path, "host", ["--deflate", "host"], where="device"), phase_cli(tmp_path, "dev", ["--deflate", "device"], where="device")
    assert read(dev) == read(host) and read(dev + ".bai") == read(host + ".bai")
    assert len(cu.block_sizes(dev)) > 5
