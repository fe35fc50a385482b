"""The rules of zmx_bitjoin_many_device's kernel (zopfli_amd/csrc/device/zmx_bitjoin.h: the tile-to-destination search, the
destination's own table, BitjoinTile on the local tile) run on the CPU by tests/hostlib/bitjoin_many_print.cc — the grid
emulated at 1 workgroup, at kBitjoinMaxBlocks and at what the driver launches, a workgroup's threads one after the other —
over the tables of tests/bitjoin_many_cases.py: the whole block of destinations and 0xA5 canaries against the big-integer
reference of tests/bitjoin_cases.py applied per destination, here and bit by bit in the program.  Then the argument rules
of host/entry_checks.h (CheckBitDests) and the packed form's arithmetic (host/device_output_plan.h) through
tests/hostlib/bitjoin_many_checks.cc."""
import os
import subprocess

import numpy as np
import pytest

import bitjoin_many_cases as mc
import oracle_lib as ol
from zopfli_amd._build import ROOT

HOSTLIB_DIR = os.path.join(ROOT, "tests", "hostlib")
BUILD = os.path.join(ROOT, "tests", "_build")
CASES = mc.cases()
GRIDS = ("1", str(mc.MAX_BLOCKS), "0")


def _make(*extra):
    subprocess.check_call(["make", "-s", "-C", HOSTLIB_DIR, "-f", "bitjoin_many.mk", *extra])


def _run(exe, tmp_path, case):
    name, _, _, dests, arena = case
    table = os.path.join(str(tmp_path), "table.txt")
    arena_file = os.path.join(str(tmp_path), "arena.bin")
    out = os.path.join(str(tmp_path), "out.bin")
    with open(table, "w") as f:
        f.write(mc.table_text(case))
    arena.tofile(arena_file)
    r = subprocess.run([exe, table, arena_file, out, *GRIDS], capture_output=True, text=True)
    assert r.returncode == 0, (name, r.stdout, r.stderr[-2000:])
    npieces = sum(len(p) for _, _, p in dests)
    assert r.stdout.split() == ["ok", str(len(dests)), str(npieces), str(sum(mc.tiles(case)))], name
    got = np.fromfile(out, dtype=np.uint8)
    want = mc.expected_block(case)
    assert len(got) == len(want), name
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (name, bad[:8])


@pytest.fixture(scope="module")
def exe():
    _make()
    return os.path.join(BUILD, "bitjoin_many_print")


@pytest.fixture(scope="module")
def checks(exe):
    return os.path.join(BUILD, "bitjoin_many_checks")


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_bitjoin_many_rules(exe, tmp_path, case):
    _run(exe, tmp_path, case)


def test_sanitized_program(tmp_path):
    """The same program under AddressSanitizer and UBSan (host code, its own main): the block of destinations is an exact
    heap block, and so is every source, so a byte written or read outside them is reported."""
    _make("SANITIZE=-fsanitize=address,undefined", "OUT_NAME=bitjoin_many_print_san")
    san = os.path.join(BUILD, "bitjoin_many_print_san")
    for case in CASES:
        _run(san, tmp_path, case)


def test_what_the_builders_reach():
    by_name = {c[0]: c for c in CASES}
    c = by_name["neighbours-5-1-27"]
    assert c[1] == 3 and [(tb + 7) // 8 for _, tb, _ in c[3]] == [5, 1, 27] and all(g == 0 for g, _, _ in c[3])
    assert mc.positions(c)[0][1] // 16 == mc.positions(c)[0][0] // 16 == mc.positions(c)[0][2] // 16      # one vector holds all three
    totals = [tb for _, tb, _ in by_name["empties"][3]]
    assert totals[0] == 0 and totals[-1] == 0 and any(a == 0 and b == 0 for a, b in zip(totals, totals[1:]))
    assert any(tb == 0 and pieces for _, tb, pieces in by_name["empties"][3])
    assert mc.tiles(by_name["one-tile"])[0] == 1 and mc.positions(by_name["one-tile"])[0][0] % 16 == 0
    assert mc.tiles(by_name["one-tile-plus-1"])[0] == 2
    assert mc.tiles(by_name["one-tile-lead-15"])[0] == 2 and mc.positions(by_name["one-tile-lead-15"])[0][0] % 16 == 15
    assert mc.tiles(by_name["three-tiles-between"]) == [1, 3, 1]
    c = by_name["many-2100"]
    assert len(c[3]) == 2100 and all(tb == 160 for _, tb, _ in c[3]) and sum(mc.tiles(c)) > mc.MAX_BLOCKS
    assert set(mc.shifts(by_name["one-bit-off"])) == {1, 31}
    assert any(nb >= 3 * 128 for _, _, ps in by_name["one-bit-off"][3] for _, _, nb, _ in ps)      # whole vectors inside a piece
    c = by_name["ragged-bits"]
    assert all(tb % 8 for _, tb, _ in c[3][:3]) and all(g == 0 for g, _, _ in c[3])
    assert by_name["gaps"][2] == 0 and by_name["gaps"][1] == 0


def _check(exe, *args):
    r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stderr)
    return r.stdout.strip()


def test_destination_table_rules(checks):
    """What zmx_bitjoin_many_device refuses of its tables before it asks the runtime anything, and the accepting case next
    to each.  Destinations are (dst, total_bits, first_piece, npieces, capacity), pieces (src, src_bit, nbits, dst_bit)."""
    pieces = [4096, 0, 10, 0, 4096, 3, 5, 10, 8192, 1, 17, 0]
    two = [100000, 15, 0, 2, 2, 100002, 17, 2, 1, 3]
    assert _check(checks, "dests", 2, 3, *two, *pieces) == "ok"
    assert _check(checks, "dests", 0, 0) == "ok"
    # a null table with a non-zero count
    assert "null destination table" in _check(checks, "dests", 2, 0)
    assert "null piece table" in _check(checks, "dests", 0, 3)
    # piece ranges that are not consecutive or leave npieces
    assert "destination 1: its pieces do not follow" in _check(checks, "dests", 2, 3, 100000, 15, 0, 2, 2, 100002, 17, 1, 1, 3, *pieces)
    assert "destination 0: its pieces do not follow" in _check(checks, "dests", 2, 3, 100000, 15, 1, 2, 2, 100002, 17, 3, 0, 3, *pieces)
    assert "destination 1: its pieces leave the table of 3" in _check(checks, "dests", 2, 3, 100000, 15, 0, 2, 2, 100002, 17, 2, 2, 3, *pieces)
    assert "the destinations take 2 pieces of 3" in _check(checks, "dests", 1, 3, 100000, 15, 0, 2, 2, *pieces)
    # a destination whose table CheckBitPieces refuses
    assert "destination 0: piece 1: it overlaps the piece before it" in _check(
        checks, "dests", 2, 3, *two, 4096, 0, 10, 0, 4096, 3, 5, 9, 8192, 1, 17, 0)
    assert "destination 1: piece 0: null pointer" in _check(checks, "dests", 2, 3, *two, 4096, 0, 10, 0, 4096, 3, 5, 10, 0, 1, 17, 0)
    assert "destination 1: total_bits 16 is below the last piece's end, 17" in _check(
        checks, "dests", 2, 3, 100000, 15, 0, 2, 2, 100002, 16, 2, 1, 3, *pieces)
    assert "destination 0: null pointer with a non-zero size" in _check(checks, "dests", 2, 3, 0, 15, 0, 2, 2, 100002, 17, 2, 1, 3, *pieces)
    assert _check(checks, "dests", 2, 3, 0, 0, 0, 0, 0, 100002, 17, 0, 3, 3, 4096, 0, 10, 0, 4096, 3, 5, 10, 4096, 9, 2, 15) == "ok"
    # a total_bits above its capacity
    assert "destination 0: total_bits 15 is above 8 * dst_capacity, 1 bytes" in _check(
        checks, "dests", 2, 3, 100000, 15, 0, 2, 1, 100002, 17, 2, 1, 3, *pieces)
    assert "destination 1: total_bits 17 is above 8 * dst_capacity, 2 bytes" in _check(
        checks, "dests", 2, 3, 100000, 15, 0, 2, 2, 100002, 17, 2, 1, 2, *pieces)
    assert _check(checks, "dests", 2, 3, 100000, 15, 0, 2, -1, 100002, 17, 2, 1, 0, *pieces) == "ok"      # a null capacity array
    # two destinations that share a byte (their bytes, not their capacities)
    assert "destination 1 overlaps destination 0" in _check(checks, "dests", 2, 3, 100000, 15, 0, 2, 2, 100001, 17, 2, 1, 3, *pieces)
    assert "destination 1 overlaps destination 0" in _check(checks, "dests", 2, 3, 100002, 15, 0, 2, 2, 100000, 17, 2, 1, 3, *pieces)
    assert _check(checks, "dests", 2, 3, 100003, 15, 0, 2, 2, 100000, 17, 2, 1, 3, *pieces) == "ok"
    # a piece whose source bytes share a byte with any destination: its own, and another one
    assert "destination 0: piece 1: destination 1 overlaps this source" in _check(
        checks, "dests", 2, 3, *two, 4096, 0, 10, 0, 100004, 3, 5, 10, 8192, 1, 17, 0)
    assert "destination 1: piece 0: destination 0 overlaps this source" in _check(
        checks, "dests", 2, 3, *two, 4096, 0, 10, 0, 4096, 3, 5, 10, 99999, 8, 8, 0)
    assert _check(checks, "dests", 2, 3, *two, 4096, 0, 10, 0, 100005, 3, 5, 10, 99997, 1, 17, 0) == "ok"    # just outside both


def test_many_destinations_against_many_pieces_is_no_product(checks, tmp_path):
    """A thousand destinations of ten pieces each: the overlap checks sort (a product would be 10^7 range pairs per
    destination table; this returns at once)."""
    dests, pieces = [], []
    for d in range(1000):
        dests += [1 << 20 | d * 64, 8 * 40, 10 * d, 10, 40]
        for i in range(10):
            pieces += [1 << 30 | (d * 10 + i) * 16, 3, 32, 32 * i]
    assert _check(checks, "dests", 1000, 10000, *dests, *pieces) == "ok"
    pieces[4 * 9999] = (1 << 20 | 500 * 64) + 39
    assert "destination 999: piece 9: destination 500 overlaps this source" in _check(checks, "dests", 1000, 10000, *dests, *pieces)


def test_packed_offsets(checks):
    """Stream i begins at the end of stream i - 1 rounded up to align; empty streams take no room."""
    sizes = [5, 0, 27, 16, 1, 0, 0, 4096, 3]
    for align in (1, 16, 4096):
        got = [int(v) for v in _check(checks, "offsets", align, *sizes).split()]
        want, end = [], 0
        for s in sizes:
            want.append((end + align - 1) // align * align)
            end = want[-1] + s
        assert got == want + [end], align
    assert _check(checks, "offsets", 1, 5, 0, 27) == "0 5 5 32"
    assert _check(checks, "offsets", 16, 5, 0, 27) == "0 16 16 43"
    assert _check(checks, "offsets", 16) == "0"
    for align in (1, 2, 16, 4096):
        assert _check(checks, "align", align) == "ok"
    for align in (0, 3, 24, 8192, 1 << 20):
        assert _check(checks, "align", align) == "bad"


@pytest.mark.skipif(not ol.have_ref(), reason="oracle/_ref not built (needs the reference's sources)")
def test_batch_bound_holds_for_random_bytes(checks):
    """zmx_compress_batch_bound against the reference's outputs for incompressible inputs — stored blocks, the worst case
    the bound is built from — packed by the offsets' rule, in all three formats."""
    ns = [0, 1, 65535, 65536, 131071, 300000, 7]
    datas = [np.random.default_rng(100 + i).integers(0, 256, n, dtype=np.uint8).tobytes() for i, n in enumerate(ns)]
    for fmt in (0, 1, 2):
        sizes = [len(ol.ref_compress(d, fmt, numiterations=1)) for d in datas]
        for align in (1, 16, 4096):
            end = int(_check(checks, "offsets", align, *sizes).split()[-1])
            bound = int(_check(checks, "bound", fmt, align, *ns))
            assert end <= bound, (fmt, align, end, bound)
            assert bound <= sum(ns) + len(ns) * (1000 + align), (fmt, align, bound)     # ... and not a useless one
