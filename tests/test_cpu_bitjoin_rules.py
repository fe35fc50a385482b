"""The rules of zmx_bitjoin_device's kernel (zopfli_amd/csrc/device/zmx_bitjoin.h: the tile-to-piece search, the walk over
a tile's pieces, the vectors inside a piece, the general per-word rule) run on the CPU by tests/hostlib/bitjoin_print.cc, a
workgroup's threads one after the other, over the tables of tests/bitjoin_cases.py: the joined bytes against the big-integer
reference here and bit by bit in the program, which also checks the guard bytes around the destination and holds every
load to the aligned words of its piece.  Then the argument rules of host/entry_checks.h and zmx_compress_bound's
arithmetic (host/device_output_plan.h) through tests/hostlib/bitjoin_checks.cc."""
import os
import subprocess

import numpy as np
import pytest

import bitjoin_cases as bc
import oracle_lib as ol
from zopfli_amd._build import ROOT

HOSTLIB_DIR = os.path.join(ROOT, "tests", "hostlib")
BUILD = os.path.join(ROOT, "tests", "_build")
CASES = bc.cases()


def _make(*extra):
    subprocess.check_call(["make", "-s", "-C", HOSTLIB_DIR, "-f", "bitjoin.mk", *extra])


def _run(exe, tmp_path, case):
    name, dst_mod, total_bits, pieces = case
    arena = bc.arena(name, pieces)
    table = os.path.join(str(tmp_path), "table.txt")
    arena_file = os.path.join(str(tmp_path), "arena.bin")
    out = os.path.join(str(tmp_path), "out.bin")
    with open(table, "w") as f:
        f.write(f"{dst_mod} {total_bits}\n")
        f.write("".join(f"{-1 if off is None else off} {sb} {nb} {db}\n" for off, sb, nb, db in pieces))
    arena.tofile(arena_file)
    r = subprocess.run([exe, table, arena_file, out], capture_output=True, text=True)
    assert r.returncode == 0, (name, r.stdout, r.stderr[-2000:])
    nbytes = (total_bits + 7) // 8
    ntiles = (dst_mod + nbytes + bc.TILE - 1) // bc.TILE if total_bits else 0
    assert r.stdout.split() == ["ok", str(len(pieces)), str(nbytes), str(ntiles)], name
    got = np.fromfile(out, dtype=np.uint8)
    assert np.array_equal(got, bc.expected(total_bits, pieces, arena)), name


@pytest.fixture(scope="module")
def exe():
    _make()
    return os.path.join(BUILD, "bitjoin_print")


@pytest.fixture(scope="module")
def checks(exe):
    return os.path.join(BUILD, "bitjoin_checks")


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_bitjoin_rules(exe, tmp_path, case):
    _run(exe, tmp_path, case)


def test_bitjoin_rules_past_the_grid(exe, tmp_path):
    """33 MiB + 5 bits: more tiles than the grid has workgroups (the program walks them all, as the grid-stride loop does)."""
    case = bc.big()
    assert (case[2] + 7) // 8 > bc.TILE * 2048
    _run(exe, tmp_path, case)


def test_sanitized_program(tmp_path):
    """The same program under AddressSanitizer and UBSan (host code, its own main): every source lies in a heap block that
    ends with the last aligned word holding one of its bits, so a read beyond what the header promises is reported."""
    _make("SANITIZE=-fsanitize=address,undefined", "OUT_NAME=bitjoin_print_san")
    san = os.path.join(BUILD, "bitjoin_print_san")
    for case in CASES:
        _run(san, tmp_path, case)


def test_what_the_builders_reach():
    """The tables hold what they are there for: every shift of the funnel, pieces inside one word, empty pieces, gaps,
    tile edges, every alignment."""
    by_name = {c[0]: c for c in CASES}
    for n in bc.SIZES:
        _, dst_mod, total, pieces = by_name[f"pairs-{n}"]
        assert {(sb % 32, db % 32) for _, sb, _, db in pieces} == {(s, d) for s in range(32) for d in range(32)}
        assert all(nb == n for _, _, nb, _ in pieces)
    # the vectors inside the 4099-bit pieces take every funnel shift 0 .. 31 (source bit address - destination bit
    # address, mod 32; the arena and the destination begin at 16-byte boundaries)
    shifts = {(8 * off + sb - db) % 32 for off, sb, nb, db in by_name["pairs-4099"][3]}
    assert shifts == set(range(32))
    assert all(nb >= 3 * 128 for _, _, nb, _ in by_name["pairs-4099"][3])   # each holds whole 16-byte vectors
    _, _, _, pieces = by_name["one-word-32"]
    assert len(pieces) == 32 and {db // 32 for _, _, _, db in pieces} == {2}
    _, _, _, pieces = by_name["empties"]
    assert sum(nb == 0 for _, _, nb, _ in pieces) >= 5 and pieces[0][2] == 0 and pieces[-1][2] == 0
    assert any(off is None for off, _, _, _ in pieces) and any(off is not None and nb == 0 for off, _, nb, _ in pieces)
    _, _, _, pieces = by_name["gaps"]
    gaps = [b[3] - (a[3] + a[2]) for a, b in zip(pieces, pieces[1:])]
    assert set(range(1, 8)) <= set(gaps) and max(gaps) >= 2 * bc.TILE_BITS
    for e in (-1, 0, 1):
        _, _, _, pieces = by_name[f"tile-edge{e:+d}"]
        assert pieces[0][3] + pieces[0][2] == bc.TILE_BITS + e == pieces[1][3]
        assert pieces[1][3] + pieces[1][2] == 2 * bc.TILE_BITS + e
    assert {(c[1], c[3][0][0] % 16) for c in CASES if c[0].startswith("align-")} == {(d, s) for d in bc.OFFSETS for s in bc.OFFSETS}
    assert {c[2] for c in CASES} >= {0, 1}


def _check(exe, *args):
    r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stderr)
    return r.stdout.strip()


def test_piece_table_rules(checks):
    """What zmx_bitjoin_device refuses of its table before it asks the runtime anything; pieces are (src, src_bit, nbits, dst_bit)."""
    ok = [4096, 0, 10, 0, 4096, 3, 5, 10, 0, 0, 0, 15, 8192, 1, 17, 15]
    assert _check(checks, "pieces", 32, 4, *ok) == "ok"
    assert _check(checks, "pieces", 0, 0) == "ok"
    assert _check(checks, "pieces", 7, 1) == "ok"                        # bits that no piece covers
    assert "piece 1: null pointer" in _check(checks, "pieces", 32, 4, 4096, 0, 10, 0, 0, 3, 5, 10)
    assert "piece 1: the pieces are not sorted" in _check(checks, "pieces", 64, 8, 4096, 0, 10, 20, 4096, 0, 5, 3)
    assert "piece 1: it overlaps the piece before it" in _check(checks, "pieces", 64, 8, 4096, 0, 10, 0, 4096, 0, 5, 9)
    assert "piece 1: it overlaps" in _check(checks, "pieces", 64, 8, 4096, 0, 10, 0, 0, 0, 0, 9)     # an empty one too
    assert "below the last piece's end, 32" in _check(checks, "pieces", 31, 4, *ok)
    assert "above 8 * dst_capacity" in _check(checks, "pieces", 33, 4, *ok)
    assert _check(checks, "pieces", 33, 5, *ok) == "ok"
    assert "piece 0: a bit count of 2^60 or more" in _check(checks, "pieces", 1 << 62, 1 << 60, 4096, 0, 1 << 60, 0)
    assert "piece 0: a bit count of 2^60 or more" in _check(checks, "pieces", 64, 8, 4096, 1 << 60, 1, 0)
    # the destination and a source apart: [dst, dst + bytes) against [lo, hi)
    assert _check(checks, "apart", 3, 1000, 100, 1100, 1200) == "ok"
    assert _check(checks, "apart", 3, 1000, 100, 900, 1000) == "ok"
    assert "piece 3: the destination overlaps this source" in _check(checks, "apart", 3, 1000, 100, 1099, 1200)
    assert "piece 3: the destination overlaps this source" in _check(checks, "apart", 3, 1000, 100, 900, 1001)


@pytest.mark.skipif(not ol.have_ref(), reason="oracle/_ref not built (needs the reference's sources)")
@pytest.mark.parametrize("n", [0, 1, 65535, 65536, 131071, 1000000, 1000001])
def test_compress_bound_holds_for_random_bytes(checks, n):
    """zmx_compress_bound against the reference's output for incompressible input — stored blocks, the worst case the
    bound is built from — in all three formats."""
    data = np.random.default_rng(n + 1).integers(0, 256, n, dtype=np.uint8).tobytes()
    for fmt in (0, 1, 2):
        size = len(ol.ref_compress(data, fmt, numiterations=1))
        bound = int(_check(checks, "bound", fmt, n))
        assert size <= bound, (n, fmt, size, bound)
        assert bound <= n + n // 1000 + 1000, (n, fmt, bound)     # ... and not a useless one
