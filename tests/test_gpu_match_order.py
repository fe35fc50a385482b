"""k_match2's order of service (zmx_set_match_order / ZOPFLI_AMD_MATCH_ORDER): a tile's positions handed out by k_hits'
estimate of their walk, longest first, or in ascending order.  The records must be the reference's either way:
ZopfliFindLongestMatch (lz77.c:407) at every position — length, distance, the whole sublen — with kernel 2 forced so
that k_match2 takes every block, on the shapes where an ordered queue can go wrong."""
import hashlib
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as ol
from zopfli_amd import generate

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (what, class, total size, blocks)
ORDER_CASES = [
    ("one_full_tile", "T", 2048, [(0, 2048)]),
    ("second_tile_of_one", "T", 2049, [(0, 2049)]),
    ("fewer_than_lanes", "T", 300, [(0, 300)]),
    ("tiny_and_empty", "M", 150000, [(0, 3), (3, 5), (5, 5)]),
    ("window_in_front", "P", 66000, [(33000, 66000)]),       # tiles not aligned with k_hits' 32768-position chunks
    ("unaligned_ws0", "X", 50000, [(20000, 50000)]),         # same, with the region starting at 0
    ("one_bucket", "R", 30000, [(0, 30000)]),
    ("top_bucket", "B", 40000, [(0, 40000)]),                # chain cap + hash switch
    ("runs_across_end", "Z", 90000, [(0, 45001), (45001, 90000)]),
]


def _mismatches(t, b, o, s, e):
    bad = []
    for pos in range(s, e):
        gl, gd, gsub = t.find_longest_match(b, pos)
        ol_, od, osub = o.find_longest_match(pos)
        same = (gl == ol_ and gd == od) if ol_ >= 3 else (gl < 3 and ol_ < 3)
        if same and ol_ >= 3:
            same = np.array_equal(gsub[3:ol_ + 1], osub[3:ol_ + 1])
        if not same:
            bad.append((pos, (gl, gd), (ol_, od)))
            if len(bad) >= 5:
                break
    return bad


@pytest.fixture()
def kernel2(gpu_ctx):
    gpu_ctx.lib.zmx_set_match_kernel(2)
    yield gpu_ctx
    gpu_ctx.lib.zmx_set_match_kernel(0)
    gpu_ctx.lib.zmx_set_match_order(1)


@pytest.mark.parametrize("case", ORDER_CASES, ids=lambda c: c[0])
def test_match_table_in_both_orders(kernel2, case):
    """Both orders against one oracle table per block."""
    _, cls, n, blocks = case
    data = generate(cls, n)
    kernel2.set_input(data)
    tabs = {}
    try:
        for order in (1, 0):
            assert kernel2.lib.zmx_set_match_order(order) == 0
            tabs[order] = kernel2.build_tables(blocks)
        for b, (s, e) in enumerate(blocks):
            o = ol.OracleTable(data, s, e)
            for order, t in tabs.items():
                bad = _mismatches(t, b, o, s, e)
                assert not bad, f"order {order}, block {b} [{s},{e}): first mismatches (pos, gpu, oracle) {bad}"
    finally:
        for t in tabs.values():
            t.free()


def test_parent_path_with_order_on(kernel2):
    """zmx_tables_build_from with the switch on: the parent is built in order, the few recomputed tiles in ascending
    order (nobody ran k_hits for them), and every sub-block's records are the reference's."""
    data = generate("T", 70000)
    blocks = [(0, 30000), (30000, 30100), (30100, 70000)]
    kernel2.set_input(data)
    assert kernel2.lib.zmx_set_match_order(1) == 0
    pt = kernel2.build_tables([(0, 70000)], matches_only=True)
    t = kernel2.build_tables(blocks, parent=pt)
    pt.free()
    try:
        for b, (s, e) in enumerate(blocks):
            bad = _mismatches(t, b, ol.OracleTable(data, s, e), s, e)
            assert not bad, f"block {b} [{s},{e}): first mismatches (pos, gpu, oracle) {bad}"
    finally:
        t.free()


def _record_bytes(l, d, sub):
    return (np.array([l if l >= 3 else 0, d if l >= 3 else 0], dtype=np.uint16).tobytes()
            + np.asarray(sub[3:l + 1] if l >= 3 else [], dtype=np.uint16).tobytes())


def _child(body, **env):
    """A fresh process with kernel 2 forced (the GPU suite's own process keeps its context)."""
    code = ("import hashlib, sys\nimport numpy as np\nsys.path.insert(0, %r)\n"
            "from zopfli_amd import Context, api, generate\n" % ROOT) + inspect.getsource(_record_bytes) + body
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ZOPFLI_AMD_MATCH="2", **env),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def test_order_under_guard():
    """T, 70 000 B, in a fresh process under ZOPFLI_AMD_GUARD=1 (red zones, poisoned bodies, a check after every
    launch): a position the order dropped is a poisoned record, one handed out twice or a slot beyond the tile a
    clobbered one — not a stale correct record left by an earlier build."""
    n = 70000
    r = _child("ctx = Context(0, api.library())\n"
               "ctx.set_input(generate('T', %d))\n"
               "t = ctx.build_tables([(0, %d)])\n"
               "h = hashlib.sha256()\n"
               "for pos in range(%d):\n"
               "    h.update(_record_bytes(*t.find_longest_match(0, pos)))\n"
               "t.free()\n"
               "ctx.close()\n"
               "print(h.hexdigest())\n" % (n, n, n), ZOPFLI_AMD_GUARD="1", ZOPFLI_AMD_MATCH_ORDER="1")
    o = ol.OracleTable(generate("T", n), 0, n)
    h = hashlib.sha256()
    for pos in range(n):
        h.update(_record_bytes(*o.find_longest_match(pos)))
    assert r.stdout.split()[-1] == h.hexdigest()


def test_switch_selects_the_order():
    """The switch reaches the kernel: under ZOPFLI_AMD_PROF every whole build reports how k_match2 handed its positions
    out.  Without this, a build that quietly passed no estimates would pass every comparison above in ascending order."""
    r = _child("lib = api.library()\n"
               "ctx = Context(0, lib)\n"
               "ctx.set_input(generate('T', 5000))\n"
               "for order in (1, 0):\n"
               "    assert lib.zmx_set_match_order(order) == 0\n"
               "    ctx.build_tables([(0, 5000)]).free()\n"
               "ctx.close()\n", ZOPFLI_AMD_PROF="1")
    said = [ln.split("positions handed out ")[1] for ln in r.stderr.splitlines() if "positions handed out " in ln]
    assert said == ["by k_hits' estimate, longest first", "in ascending order"], r.stderr[-2000:]
