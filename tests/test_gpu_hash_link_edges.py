"""k_same and k_chain (zmx_kernels.h) where they decide something — the 65535 cap of same[], links exactly at and just
past the 32767 window, chunk seams and the chunk's last position (k_chain's own "none" as a relative index), steps of 64
positions that share a key, the zero fill past a block end, windowstart at every alignment — against the real
reference's hash state (tests/hash_link_cases.py: reference_links, the cases and why each is there), and k_match2, the
kernel that walks those links, against the oracle at every position of the same inputs.  Tables built from a parent
compute the links only near the block ends and cannot be downloaded: there the match records of sub-blocks that end
inside, just after and wholly within runs longer than the cap speak for them.

tests/test_cpu_hash_link_cases.py shows on the CPU that every case reaches its edge and that the oracle's links are
the reference's on all of them; where oracle/_ref was not built the links here are checked against the oracle's."""
import ctypes
import functools

import numpy as np
import pytest

import hash_link_cases as hc
import oracle_lib as ol

pytestmark = pytest.mark.gpu
_u16p = ctypes.POINTER(ctypes.c_uint16)


def _first_diff(a, b):
    n = min(len(a), len(b))
    idx = np.nonzero(np.asarray(a[:n]) != np.asarray(b[:n]))[0]
    return int(idx[0]) if len(idx) else n


def _expected_links(name, b):
    if ol.have_ref():
        return hc.links(name, b)
    c = hc.case(name)
    return ol.OracleTable(c.data, *c.blocks[b]).hash_links()


@pytest.mark.parametrize("name", hc.CASES)
def test_links_vs_reference(gpu_ctx, name):
    """Tables.hash_links == the reference's same[], prev1[], prev2[] over every block's windowstart .. inend - 1, under
    the default match-kernel setting (k_same and k_chain run under every setting)."""
    c = hc.case(name)
    gpu_ctx.set_input(c.data)
    t = gpu_ctx.build_tables(c.blocks, matches_only=True)
    try:
        for b, (s, e) in enumerate(c.blocks):
            if e == s:
                continue
            got = t.hash_links(b)
            want = _expected_links(name, b)
            for what, g, w in zip(("same", "prev1", "prev2"), got, want):
                i = _first_diff(g, w)
                assert len(g) == len(w) and i == len(w), \
                    f"{name} block {b} [{s},{e}) {what}: first diff at region index {i}: gpu {g[i]}, reference {w[i]}"
    finally:
        t.free()


@functools.lru_cache(maxsize=None)
def _oracle_records(data, s, e):
    """ZopfliFindLongestMatch at every position of block [s, e) as the oracle gives it: (length, distance,
    sublen[3 .. length] as bytes), None where there is no match of 3 or more.  Computed once per block."""
    o = ol.OracleTable(data, s, e)
    sub = (ctypes.c_uint16 * 259)()
    d, l = ctypes.c_uint16(0), ctypes.c_uint16(0)
    fn, h, rd, rl = o.lib.zo_find_longest_match, o.h, ctypes.byref(d), ctypes.byref(l)
    view = memoryview(sub).cast("B")
    out = []
    for pos in range(s, e):
        fn(h, pos, sub, rd, rl)
        n = l.value
        out.append((n, d.value, bytes(view[6:2 * n + 2])) if n >= 3 else None)
    o.close()
    return out


def _gpu_records(ctx, t, b, s, e):
    """The same from zmx_find_longest_match (by the rule of test_match_table: below 3 there is no match to compare)."""
    sub = (ctypes.c_uint16 * 259)()
    d, l = ctypes.c_uint16(0), ctypes.c_uint16(0)
    fn, rd, rl = ctx.lib.zmx_find_longest_match, ctypes.byref(d), ctypes.byref(l)
    view = memoryview(sub).cast("B")
    out = []
    for pos in range(s, e):
        ctx._check(fn(ctx.handle, t.handle, b, pos, sub, rd, rl), "zmx_find_longest_match")
        n = l.value
        out.append((n, d.value, bytes(view[6:2 * n + 2])) if n >= 3 else None)
    return out


def _assert_records(ctx, t, data, blocks, label):
    for b, (s, e) in enumerate(blocks):
        got = _gpu_records(ctx, t, b, s, e)
        want = _oracle_records(data, s, e)
        if got != want:
            bad = [(s + i, g and g[:2], w and w[:2]) for i, (g, w) in enumerate(zip(got, want)) if g != w][:5]
            raise AssertionError(f"{label} block {b} [{s},{e}): first mismatches (pos, gpu, oracle) {bad}")


@pytest.mark.parametrize("name", hc.MATCH_CASES)
def test_match2_vs_oracle(gpu_ctx, name):
    """k_match2 (forced) on k_same's and k_chain's links == ZopfliFindLongestMatch: length, distance and
    sublen[3 .. length] at every position."""
    c = hc.case(name)
    gpu_ctx.set_input(c.data)
    gpu_ctx.lib.zmx_set_match_kernel(2)
    try:
        t = gpu_ctx.build_tables(c.blocks, matches_only=True)
    finally:
        gpu_ctx.lib.zmx_set_match_kernel(0)
    try:
        _assert_records(gpu_ctx, t, c.data, c.blocks, name)
    finally:
        t.free()


@pytest.mark.parametrize("kernel", [0, 2], ids=["default", "match2"])
@pytest.mark.parametrize("matches_only", [True, False], ids=["parent_matches_only", "parent_full"])
def test_reuse_at_long_runs(gpu_ctx, matches_only, kernel):
    """Tables built from a parent (0, n) over run-cap-c's input (runs of 100000 and 70000 bytes): sub-blocks that end
    inside a run MT k - 1, MT k and MT k + 1 after its start, one byte after a run's end, that are one run from before
    their windowstart to their inend, that are 300 bytes of a run; and one whose recomputed tiles lie so far up that
    k_chain skips chunks and k_same what is below their warm-up.  Every position's record == the oracle's; the partial
    hash arrays are refused."""
    c = hc.case("run-cap-c")
    n = len(c.data)
    gpu_ctx.set_input(c.data)
    gpu_ctx.lib.zmx_set_match_kernel(kernel)
    try:
        for label, blocks in hc.REUSE_SUBBLOCKS.items():
            # (a parent of its own for every list: the tables built from it take over its change-point pool)
            pt = gpu_ctx.build_tables([(0, n)], matches_only=matches_only)
            t = gpu_ctx.build_tables(blocks, parent=pt)
            pt.free()
            try:
                _assert_records(gpu_ctx, t, c.data, blocks, label)
                with pytest.raises(Exception, match="only near the block ends"):
                    t.hash_links(0)
            finally:
                t.free()
    finally:
        gpu_ctx.lib.zmx_set_match_kernel(0)
