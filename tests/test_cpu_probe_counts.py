"""The counting rules of the device-input path (zopfli_amd/csrc/device/zmx_probe.h: what k_probe_counts and k_tail_runs
compute) run on the CPU by tests/hostlib/probe_print.cc, against zamd::MasterBlockCost and zamd::LooksLikeRuns of the host
library (their own loops over the bytes) and against a plain Python walk for the tail runs.  Doubles are compared by
their bits."""
import ctypes
import os
import struct
import subprocess

import pytest

import device_input_cases as cases
from zopfli_amd._build import ROOT
from zopfli_amd.datagen import generate

HOSTLIB_DIR = os.path.join(ROOT, "tests", "hostlib")
BUILD = os.path.join(ROOT, "tests", "_build")


def _make(*extra):
    subprocess.check_call(["make", "-s", "-C", HOSTLIB_DIR, "-f", "probe.mk", *extra])


@pytest.fixture(scope="module")
def probe():
    _make()
    exe = os.path.join(BUILD, "probe_print")

    def run(tmp_path, data, ranges, exe=exe):
        path = os.path.join(str(tmp_path), "input.bin")
        with open(path, "wb") as f:
            f.write(data)
        args = [str(v) for r in ranges for v in r]
        out = subprocess.run([exe, path] + args, check=True, capture_output=True, text=True).stdout.split("\n")
        rows = []
        for line in out[:len(ranges)]:
            w = line.split()
            rows.append({"counts": [int(x) for x in w[:5]], "cost": int(w[5], 16), "runs": int(w[6]), "tail": int(w[7])})
        assert len(rows) == len(ranges)
        return rows
    return run


@pytest.fixture(scope="module")
def host():
    """zamd::MasterBlockCost(in, begin, end) -> the double's bits, zamd::LooksLikeRuns(in, lo, hi) of the host library."""
    subprocess.check_call(["make", "-s", "-C", HOSTLIB_DIR])
    lib = ctypes.CDLL(os.path.join(BUILD, "libzopfli_hosttest.so"))
    cost = getattr(lib, "_ZN4zamd15MasterBlockCostEPKhmm")
    cost.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t]
    cost.restype = ctypes.c_double
    runs = getattr(lib, "_ZN4zamd13LooksLikeRunsEPKhmm")
    runs.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t]
    runs.restype = ctypes.c_bool

    def bits(data, b, e):
        return struct.unpack("<Q", struct.pack("<d", cost(data, b, e)))[0]
    return bits, lambda data, b, e: int(bool(runs(data, b, e)))


def _master_blocks(n):
    return [(b, min(n, b + cases.MASTER_BLOCK)) for b in range(0, max(n, 1), cases.MASTER_BLOCK)]


def test_seam_sizes(probe, host, tmp_path):
    """The last probe against `i + 64 <= end`, and probes at a master-block seam: every prefix as a whole and as its
    master blocks."""
    cost, runs = host
    data = cases.mixed(2000064)
    ranges = []
    for n in cases.SEAM_SIZES:
        ranges += [(0, n)] + _master_blocks(n)
    rows = probe(tmp_path, data, ranges)
    some_runs = some_few = False
    for (b, e), row in zip(ranges, rows):
        assert row["cost"] == cost(data, b, e), (b, e)
        assert row["runs"] == runs(data, b, e), (b, e)
        want_probes = 0 if e - b < 64 else (e - b - 64) // 1024 + 1
        assert row["counts"][0] == want_probes and row["counts"][3] == (want_probes + 3) // 4, (b, e)
        some_runs |= row["counts"][1] > 0
        some_few |= row["counts"][2] > 0
    assert some_runs and some_few


def test_crafted_probes(probe, host, tmp_path):
    """Runs of exactly 63 and 64 equal bytes, exactly 4 and 5 distinct values (values that differ only in bits 6-7
    among them): every probe alone, and all of them as one range."""
    cost, runs = host
    data, want = cases.crafted_probes()
    ranges = [(1024 * k, 1024 * k + 64) for k in range(len(want))] + [(0, len(data))]
    rows = probe(tmp_path, data, ranges)
    for k, (is_run, is_few) in enumerate(want):
        assert rows[k]["counts"][:3] == [1, is_run, is_few], k
    assert rows[-1]["counts"][:3] == [len(want), sum(w[0] for w in want), sum(w[1] for w in want)]
    for (b, e), row in zip(ranges, rows):
        assert row["cost"] == cost(data, b, e) and row["runs"] == runs(data, b, e), (b, e)


@pytest.mark.parametrize("hits,want", [(1, 0), (2, 1)])
def test_runs_threshold(probe, host, tmp_path, hits, want):
    """200 probes of the 4096 stride: one hit is below 1 % of them, two hits are exactly 1 %."""
    data = cases.runs_threshold(hits)
    row = probe(tmp_path, data, [(0, len(data))])[0]
    assert row["counts"][3:] == [200, hits]
    assert row["runs"] == want == host[1](data, 0, len(data))
    assert row["cost"] == host[0](data, 0, len(data))


def test_tail_runs(probe, tmp_path):
    """TailRunStart against the plain walk: runs of 1 ... 65 601 bytes at a block's end, and a run that reaches the
    block's start."""
    text = generate("T", cases.TAIL_PARENT)
    for run in cases.TAIL_RUNS + [None]:
        data, blocks, want = cases.tail_case(text, run)
        rows = probe(tmp_path, data, blocks)
        child = blocks[-2]
        assert cases.tail_run_start(data, *child) == want, run
        for (s, e), row in zip(blocks, rows):
            assert row["tail"] == cases.tail_run_start(data, s, e), (run, s, e)


def test_sanitized_program(probe, tmp_path):
    """The same program under AddressSanitizer and UBSan (host code, its own main): probes that end exactly at the end
    of an exact-size heap copy, and the longest tail walk."""
    _make("SANITIZE=-fsanitize=address,undefined", "OUT_NAME=probe_print_san")
    exe = os.path.join(BUILD, "probe_print_san")
    data = cases.mixed(4160)
    ranges = [(0, n) for n in (0, 63, 64, 65, 1087, 1088, 4159, 4160)]
    assert probe(tmp_path, data, ranges, exe=exe) == probe(tmp_path, data, ranges)
    data, blocks, _ = cases.tail_case(generate("T", cases.TAIL_PARENT), 65601)
    assert probe(tmp_path, data, blocks, exe=exe) == probe(tmp_path, data, blocks)
