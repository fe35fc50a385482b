"""The hash-link cases of tests/hash_link_cases.py on the CPU: the oracle's same[], prev1[], prev2[] (a backward
recurrence and a head table over whole positions, oracle/zopfli_oracle.c) == the real reference's hash state replayed
update by update (hash.c's forward loop and its 32768-slot ring), on inputs with runs at and past the 65535 cap,
positions of one hash value exactly a window apart, periods that fill a step with one key and blocks that end inside
the input.  And every case reaches what it is named for, by the reference's links alone — a case that stopped reaching
its edge would make the GPU test (test_gpu_hash_link_edges.py) pass for nothing."""
import time

import numpy as np
import pytest

import hash_link_cases as hc
import oracle_lib as ol

pytestmark = pytest.mark.skipif(not ol.have_ref(), reason="oracle/_ref not built")


def _first_diff(a, b):
    idx = np.nonzero(np.asarray(a) != np.asarray(b))[0]
    return int(idx[0]) if len(idx) else -1


@pytest.mark.parametrize("name", hc.CASES)
def test_oracle_links_vs_reference(name):
    """OracleTable.hash_links() == reference_links() in all three arrays, every block of every case."""
    c = hc.case(name)
    t_ref = t_oracle = 0.0
    for b, (s, e) in enumerate(c.blocks):
        if e == s:
            continue
        t0 = time.perf_counter()
        want = hc.links(name, b)
        t1 = time.perf_counter()
        got = ol.OracleTable(c.data, s, e).hash_links()
        t_ref += t1 - t0
        t_oracle += time.perf_counter() - t1
        for what, g, w in zip(("same", "prev1", "prev2"), got, want):
            assert np.array_equal(g, w), f"{name} block {b} [{s},{e}) {what}: first diff at region index {_first_diff(g, w)}"
    print(f"{name}: {len(c.data)} bytes, {len(c.blocks)} blocks: replay {t_ref:.2f} s (0 if another test made it), "
          f"oracle {t_oracle:.2f} s")


def _family(fam):
    return {n: hc.reach(n) for n in hc.FAMILIES[fam]}


def test_run_cap_reaches_the_cap():
    f = _family("run-cap")
    stretches = sum((r["capped_stretches"] for r in f.values()), [])
    # following equal bytes exactly 65534: the run starts with same == 65534; exactly 65535, 65536, 65537: with
    # 65535, held for 1, 2 and 3 positions; the 100000-byte run holds it for 100000 - 65535 positions
    assert 65534 in f["run-cap-a"]["run_start_same"] and 65535 in f["run-cap-a"]["run_start_same"]
    assert sorted(f["run-cap-a"]["capped_stretches"]) == [1]
    assert sorted(f["run-cap-b"]["capped_stretches"]) == [2, 3]
    assert max(stretches) == 100000 - 65535 and max(stretches) > 64
    # windowstart inside the capped part of a run: the region's first position is capped
    c = hc.case("run-cap-c")
    assert hc.links("run-cap-c", 1)[0][0] == 65535 and hc.windowstart(c.blocks[1][0]) > 0
    # a run from the window before instart through inend: same[] counts down to 0 at inend - 1 from before instart
    s, e = c.blocks[2]
    same = hc.links("run-cap-c", 2)[0].astype(np.int64)
    i0 = hc.RUN_C["run1"][0] - hc.windowstart(s)
    assert i0 < s - hc.windowstart(s) and np.array_equal(same[i0:], np.arange(e - hc.RUN_C["run1"][0] - 1, -1, -1))
    # a k_chain step (64 positions from a multiple of 64) whose second-chain keys are all one value
    assert f["run-cap-d"]["uniform_step2"] >= (100000 - 65535) // 64 - 1
    assert f["run-cap-c"]["uniform_step2"] > 0


def test_run_scan_reaches_every_alignment():
    f = hc.reach("run-scan")
    assert f["scan_pairs"] >= {(off, r) for off in range(8) for r in range(24)}
    assert f["ws_mod8"] >= set(range(1, 8))
    assert any(ws % 2 for ws in (hc.windowstart(s) for s, _ in hc.case("run-scan").blocks))
    assert f["end_j"] >= set(range(9)) and f["cut_by_inend"] >= 2
    for b, ends in f["end_mod64"].items():
        assert ends >= {63, 0, 1}, b
    assert len(f["end_mod64"]) == 10


def test_window_edge_reaches_the_edge():
    f = _family("window-edge")
    for name, r in f.items():
        for ch in (1, 2):
            assert r["links"][ch] >= {32766, 32767}, (name, ch)
            # a link of 0 where the key's nearest earlier position is exactly 32768 and 32769 back
            assert r["zero_at"][ch] >= {32768, 32769}, (name, ch)
        # every planted pair is what it was planted as: nothing of its key between the two, and the link is d or none
        for (b, i, d), (true1, true2, p1, p2, same) in r["pairs"].items():
            want = d if d <= 32767 else 0
            assert (true1, true2, p1, p2, same) == (d, d, want, want, 0), (name, b, i, d)
        for (b, i, d), (true1, true2, p1, p2, same) in r["run_pairs"].items():
            assert same >= 3 and true2 == d and p2 == (d if d <= 32767 else 0) and true1 != true2, (name, b, i, d)
    placed = {n: {(i, d) for (_, i, d) in list(r["pairs"]) + list(r["run_pairs"])} for n, r in f.items()}

    def chunk(i):
        return i // 32768

    every = set().union(*placed.values())
    for d in (32766, 32767):         # a pair inside one chunk (wider pairs cannot be)
        assert any(dd == d and chunk(i) == chunk(i + d) for i, dd in every), d
    for d in (32766, 32767, 32768, 32769):
        for seam in (32768, 65536):  # a pair across each seam
            assert any(dd == d and i < seam <= i + d < seam + 32768 for i, dd in every), (d, seam)
        # the first marker at region index 0, the last at the block's last full position
        b = [k for k, (_, dd) in enumerate(hc.EDGE_ENDS) if dd == d][0]
        s, e = hc.case("window-edge-ends").blocks[b]
        assert (b, 0, d) in f["window-edge-ends"]["pairs"] and e - hc.windowstart(s) - 3 == d
    # markers at region indices 65535 (a full chunk's last position: k_chain's "none" as a relative index), 65536, 65537
    for i in (65535, 65536, 65537):
        assert any(a + d == i for a, d in every), i
    assert (32768, 32767) in placed["window-edge-b"] and (32768, 32767) in placed["window-edge-runs"]
    # runs of equal same 32767 apart, and of different same
    assert (200, 32767) in placed["window-edge-runs"]
    assert any(m1 != m2 and d == 32767 for _, d, m1, m2 in hc.EDGE_RUNS["runs"])


def test_step_groups_fill_steps():
    f = hc.reach("step-groups")
    assert f["warm_group"] >= 3 and f["emit_group"] == 64
    for s, e in hc.case("step-groups").blocks:
        assert e - hc.windowstart(s) > 65536


def test_block_end_zeros_link_through_the_zero_fill():
    c = hc.case("block-end-zeros")
    f = hc.reach("block-end-zeros")
    for (b, l2, l1), (s, e), at in zip(f["end_links"], c.blocks, c.facts["plants"]):
        assert e < len(c.data) and c.data[e] != 0 and c.data[e + 1] != 0
        assert l2 == e - 2 - at and l1 == e - 1 - (at + 1), (b, l2, l1)
        # the same positions when the hash sees the true following bytes: no link
        ws = hc.windowstart(s)
        true = hc.reference_links(c.data, s, len(c.data))[1]
        assert true[e - 2 - ws] == 0 and true[e - 1 - ws] == 0, b
    assert hc.windowstart(c.blocks[2][0]) < c.facts["plants"][2] < c.blocks[2][0]    # one plant in the window


def test_mixed_lengths_shapes():
    c = hc.case("mixed-lengths")
    sizes = [e - hc.windowstart(s) for s, e in c.blocks]
    assert min(sizes) < hc.STEP and 0 in [e - s for s, e in c.blocks] and max(sizes) > 3 * 32768
    assert c.data == hc.case("run-cap-c").data


def test_reuse_subblocks_sit_where_they_say():
    """The sub-block lists of the GPU reuse test: ends MT k - 1, MT k, MT k + 1 into a run longer than 65535 + MT, an
    end one byte after a run, a sub-block that is one run from before its windowstart, 300 bytes inside a run."""
    data = np.frombuffer(hc.case("run-cap-c").data, dtype=np.uint8)
    (a0, a1), (b0, b1) = hc.RUN_C["run0"], hc.RUN_C["run1"]
    assert a1 - a0 > 65535 + hc.MT and b1 - b0 > 65535 + hc.MT
    assert (data[a0:a1] == 0).all() and data[a0 - 1] != 0 and data[a1] != 0
    assert (data[b0:b1] == 255).all() and data[b0 - 1] != 255 and data[b1] != 255
    subs = hc.REUSE_SUBBLOCKS["ends-in-run"]
    assert {(e - a0) % hc.MT for _, e in subs[:3]} == {hc.MT - 1, 0, 1} and all(a0 < e < a1 for _, e in subs[:3])
    assert subs[3][1] - subs[3][0] == 300 and a0 < subs[3][0] and subs[3][1] < a1
    assert subs[4][1] == a1 + 1
    s, e = subs[6]
    assert b0 <= hc.windowstart(s) and e <= b1
    for lst in hc.REUSE_SUBBLOCKS.values():
        assert lst[0][0] == 0 and lst[-1][1] == len(data) and all(x[1] == y[0] for x, y in zip(lst, lst[1:]))
    # the second list's first sub-block: its recomputed tiles start a chunk and more above the region's start
    s, e = hc.REUSE_SUBBLOCKS["skips-chunks"][0]
    assert (b0 - s) // hc.MT * hc.MT > 2 * 32768 and b0 < e < b1
