"""csrc/gru_tiles.h - the tile heights of the BiGRU launches - without a device: tests/host/gru_tiles_check.cpp is built once with g++
under AddressSanitizer and UBSan and run as a child process per case.  What is asserted is the rule as gru_tiles.h states it: whole
rounds of 32-site tiles (one round = 16 sites per compute unit), and the remainder as 32-site tiles if it fills more than 3/4 of a
round, else as 16-site tiles."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ranges(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gru_tiles") / "gru_tiles_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "clairs_to_amd", "csrc"), os.path.join(ROOT, "tests", "host", "gru_tiles_check.cpp"),
                           "-o", exe])

    def run(cus, B):
        r = subprocess.run([exe, str(cus), str(B)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr.decode(errors="replace")[-2000:])
        return [tuple(int(v) for v in line.split()) for line in r.stdout.decode().splitlines()]
    return run


def batches(cus):
    rnd = 16 * cus
    return sorted({0, 1, 15, 16, rnd - 1, rnd, rnd + 1, 3 * rnd // 4, 3 * rnd // 4 + 1, 5000, 7500})


@pytest.mark.parametrize("cus", [256, 1])
def test_ranges_tile_the_batch(ranges, cus):
    rnd = 16 * cus
    for B in batches(cus):
        got = ranges(cus, B)
        # [0, B) exactly once and in order, no empty range
        at = 0
        for begin, end, ms in got:
            assert begin == at and end > begin and ms in (1, 2), (cus, B, got)
            at = end
        assert at == B, (cus, B, got)
        # whole rounds as 32-site tiles in one range; only the remainder may come as 16-site tiles, and does exactly when it fills at most
        # 3/4 of a round
        rest = B % rnd
        assert len(got) == (B >= rnd) + (rest > 0), (cus, B, got)
        assert all(ms == 2 for _, _, ms in got[:-1]), (cus, B, got)
        if B >= rnd:
            assert got[0] == (0, B - rest, 2), (cus, B, got)
        if rest:
            assert got[-1] == (B - rest, B, 1 if 4 * rest <= 3 * rnd else 2), (cus, B, got)
