"""The rules of zmx_gather_device's kernel (zopfli_amd/csrc/device/zmx_gather.h: the tile-to-piece search, the walk over
a tile's pieces, the copy of a span) run on the CPU by tests/hostlib/gather_print.cc, a workgroup's threads one after the
other, over the table of tests/gather_cases.py: the gathered bytes against numpy's concatenation here and against memcpy
in the program, which also checks the guard bytes around the destination and that no source changed."""
import os
import subprocess

import numpy as np
import pytest

import gather_cases as gc
from zopfli_amd._build import ROOT

HOSTLIB_DIR = os.path.join(ROOT, "tests", "hostlib")
BUILD = os.path.join(ROOT, "tests", "_build")
CASES = gc.cases()


def _make(*extra):
    subprocess.check_call(["make", "-s", "-C", HOSTLIB_DIR, "-f", "gather.mk", *extra])


def _run(exe, tmp_path, dst_mod, pieces):
    table = os.path.join(str(tmp_path), "table.txt")
    out = os.path.join(str(tmp_path), "out.bin")
    with open(table, "w") as f:
        f.write(f"{dst_mod}\n" + "".join(f"{s} {n}\n" for s, n in pieces))
    r = subprocess.run([exe, table, out], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    total = sum(n for _, n in pieces)
    assert r.stdout.split() == ["ok", str(len(pieces)), str(total), str((total + gc.TILE - 1) // gc.TILE)]
    return np.fromfile(out, dtype=np.uint8)


@pytest.fixture(scope="module")
def exe():
    _make()
    return os.path.join(BUILD, "gather_print")


@pytest.mark.parametrize("name,dst_mod,pieces", CASES, ids=[c[0] for c in CASES])
def test_gather_rules(exe, tmp_path, name, dst_mod, pieces):
    got = _run(exe, tmp_path, dst_mod, pieces)
    assert np.array_equal(got, gc.expected(pieces)), name


def test_every_destination_offset(exe, tmp_path):
    """The length table behind every destination offset mod 16."""
    pieces = [((5 * i) % 16, n) for i, n in enumerate(gc.LENGTHS)]
    want = gc.expected(pieces)
    for dst_mod in range(16):
        assert np.array_equal(_run(exe, tmp_path, dst_mod, pieces), want), dst_mod


def test_sanitized_program(tmp_path):
    """The same program under AddressSanitizer and UBSan (host code, its own main): every source lies in a heap block
    that ends with the last aligned word holding one of its bytes, so a read beyond what the header promises is
    reported."""
    _make("SANITIZE=-fsanitize=address,undefined", "OUT_NAME=gather_print_san")
    san = os.path.join(BUILD, "gather_print_san")
    for name, dst_mod, pieces in CASES:
        if name.startswith("alone-") and pieces[0][1] > 65:
            continue   # (the long pieces are in "lengths")
        assert np.array_equal(_run(san, tmp_path, dst_mod, pieces), gc.expected(pieces)), name
