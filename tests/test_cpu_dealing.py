"""The planning functions of the dealer (zopfli_amd/csrc/host/deal.h: LooksLikeRuns, ShardRanges, ShardPriorities,
UploadAfter) through tests/hostlib/deal_print.cc, a plain C++ program: they touch no context and read no environment.
CPU only; integers."""
import os
import subprocess

import pytest

from zopfli_amd import generate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEAL_PRINT = os.path.join(ROOT, "tests", "_build", "deal_print")


@pytest.fixture(scope="module")
def deal():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "hostlib"), "deal_print"])

    def run(*args):
        out = subprocess.run([DEAL_PRINT] + [str(a) for a in args], capture_output=True, text=True, check=True).stdout
        return [int(x) for x in out.split()]
    return run


def lst(values):
    return ",".join(str(v) for v in values)


@pytest.mark.parametrize("device_of,want", [([0, 0, 0], [1, 0, -1]), ([0, 0], [1, -1]), ([0, 1], [0, 0]),
                                            ([0, 0, 1, 1], [1, -1, 1, -1]), ([0], [0])])
def test_shard_priorities(deal, device_of, want):
    assert deal("priorities", lst(device_of)) == want


@pytest.mark.parametrize("device_of,want", [([0, 0, 0], [-1, 0, 1]), ([0, 1, 0], [-1, -1, 0])])
def test_upload_after(deal, device_of, want):
    assert deal("after", lst(device_of)) == want


def test_shard_ranges_by_weight(deal):
    assert deal("ranges", 100, 3, "28,36,36") == [0, 28, 64, 100]
    assert deal("ranges", 3, 3, "1,0,0") == [0, 1, 2, 3]              # no shard is empty
    assert deal("ranges", 10, 3, "0,0,1") == [0, 1, 2, 10]


def test_shard_ranges_ignore_unusable_weights(deal):
    equal = deal("ranges", 100, 3, "-")
    assert equal == [0, 33, 66, 100]
    assert deal("ranges", 100, 3, "28,36") == equal                   # too few
    assert deal("ranges", 100, 3, "0,0,0") == equal                   # a zero sum
    by_cost = deal("ranges", 6, 2, "-", "1,1,1,1,1,5")
    assert by_cost == [0, 5, 6]
    assert deal("ranges", 6, 2, "7", "1,1,1,1,1,5") == by_cost
    assert deal("ranges", 6, 2, "1,1", "1,1,1,1,1,5") == [0, 3, 6]    # the weights override the costs


@pytest.mark.parametrize("ndev", [1, 2, 3, 4])
@pytest.mark.parametrize("extra", [0, 1, 2, 3])
@pytest.mark.parametrize("weights", ["-", "1,0,0,0", "5,1,1,9", "0,0,0,1"])
@pytest.mark.parametrize("costly", [False, True])
def test_shard_ranges_cover_the_parts(deal, ndev, extra, weights, costly):
    """Contiguous, all parts, ndev shards, none empty — by count, by cost and by weight."""
    nparts = ndev + extra
    args = ["ranges", nparts, ndev, weights]
    if costly:
        args.append(lst([1] * (nparts - 1) + [9]))
    first = deal(*args)
    assert len(first) == ndev + 1 and first[0] == 0 and first[-1] == nparts
    assert all(a < b for a, b in zip(first, first[1:])), first


def test_looks_like_runs(deal, tmp_path):
    def runs(data):
        path = tmp_path / "in.bin"
        path.write_bytes(data)
        return deal("runs", path) == [1]
    assert runs(bytes(1 << 20))
    assert not runs(generate("R", 1 << 20))
    # a probe every 4096 bytes that has 64 bytes after it; one hit in 100 probes is 1 %, one in 101 is not
    noise = generate("R", 101 * 4096)
    assert b"\0" * 8 not in noise
    planted = bytearray(noise)
    planted[50 * 4096:50 * 4096 + 64] = bytes(64)
    assert runs(bytes(planted[:99 * 4096 + 64]))                       # exactly 100 probes
    assert not runs(bytes(planted[:100 * 4096 + 64]))                  # 101 probes
    assert not runs(bytes(63))
    assert runs(bytes(64))
