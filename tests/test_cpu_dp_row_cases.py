"""dp_row_cases.py without a device: the reference layout is held to the real algorithm — GetBestLengths walked over
its rows, each edge weighed through its code, gives the oracle's zo_get_best_lengths length array — and every case
builder is held to what it was built to reach, so that a later change to a builder cannot quietly stop reaching it.
Integer equality throughout."""
import numpy as np
import pytest

import dp_row_cases as dc
import oracle_lib as ol
from zopfli_amd import generate


# ------------------------------------------------------------------------------------------------ the reference itself
def _self_check_inputs():
    c = dc.case("shortcut")
    return {"text": (generate("T", 3600), 300, 3300), "long_run": (c.data,) + c.blocks[0]}


@pytest.mark.parametrize("model", ["entropy", "fixed"])
@pytest.mark.parametrize("what", ["text", "long_run"])
def test_reference_rows_give_the_oracles_length_array(what, model):
    """3 000 positions of class T and the 2 800 positions around two long runs (block 0 of the shortcut case: its
    shortcut positions take squeeze.c:251-271), an entropy cost model (of the block's greedy parse) and the fixed
    tree's: with codes for every row, best_lengths over reference_layout equals zo_get_best_lengths cell for cell."""
    data, s, e = _self_check_inputs()[what]
    o = ol.OracleTable(data, s, e)
    ll, d = dc.fixed_tree_costs() if model == "fixed" else ol.entropy_costs(ol.histogram(*o.greedy()))
    mincost = ol.model_min_cost(ll, d)
    want, _, _ = o.squeeze_run(ll, d, mincost)
    lay = dc.reference_layout(data, s, e, codeless=False)
    if what == "long_run":
        assert lay["shortcut"].sum() > 500
    got = dc.best_lengths(lay, ll, d, mincost)
    bad = np.flatnonzero(got[1:] != want[1:])
    assert len(bad) == 0, f"length_array differs first at cell {int(bad[0]) + 1}: {got[bad[0] + 1]}, oracle {want[bad[0] + 1]}"


def test_codeless_rows_take_no_slots():
    """The two layouts of a case differ only in the rows that lose their codes: kend and the other flags are the same,
    and with codeless off no row is codeless."""
    for name in ("kend_cut", "not_run_rows"):
        assert any(on["codeless"].any() for on in dc.layouts(name, True))
        for on, off in zip(dc.layouts(name, True), dc.layouts(name, False)):
            assert not off["codeless"].any()
            assert np.array_equal(on["flags"] & ~np.uint32(1 << 26), off["flags"])
            assert np.array_equal(on["lay"], np.where(on["codeless"] != 0, 0, off["lay"]))
            assert on["block_edges"] == int(on["lay"].sum()) and off["block_edges"] == int(off["kend"].sum())
            assert (on["block_edges"] < off["block_edges"]) == bool(on["codeless"].any())


# ------------------------------------------------------------------------------------------------ what the builders reach
def test_block_shapes():
    sizes = [e - s for s, e in dc.case("shapes").blocks]
    for around in (64, 1024, 2048):
        assert {around - 1, around, around + 1} <= set(sizes)
    assert {0, 1, 2, 3, 96, 97, 4096} <= set(sizes)
    blocks = dc.case("multi").blocks
    assert any(s == e for s, e in blocks[1:-1]) and blocks[-1][0] > 32768
    first = dc.layouts("multi", True)[-1]
    assert first["length"][0] >= 3 and first["dist"][0] > 0          # a match into the window at the block's first position
    assert all(e <= dc.MULTI_PARENT[0][1] and s >= dc.MULTI_PARENT[0][0] for s, e in blocks)
    for name in dc.CASES:
        c = dc.case(name)
        assert len(c.data) <= 200 << 10 and len(c.blocks) <= 16


def test_kend_cut_by_the_block_end():
    fall = [258, 258] + list(range(258, 2, -1)) + [1, 1]
    per, run = dc.layouts("kend_cut", True)
    for lay in (per, run):
        assert lay["kend"][-260:].tolist() == fall
        assert np.all(lay["ncp"][-260:-2] == 1)
    assert np.all(per["dist"][-260:-2] == 2) and not per["run_row"][-260:].any() and not per["codeless"].any()
    assert np.all(run["run_row"][-260:-2] == 1)
    assert np.array_equal(run["codeless"][-260:], (np.array(fall) >= 64).astype(np.uint32))      # 64 | 63
    B = len(run["kend"])
    # where the block end cuts the rows kend + u is the same for a whole window, B - 32 w: windows on either side of both
    # ends of the cell registers follow each other (test_window_kinds has the windows that cross them inside)
    reach = run["kend"].astype(np.int64) + np.arange(B) % 32
    per_window = [set(reach[32 * w:32 * w + 32].tolist()) for w in range((B - 258) // 32 + 1, B // 32)]
    assert all(len(r) == 1 for r in per_window)
    values = sorted(r.pop() for r in per_window)
    assert values[0] < 64 <= values[1] < values[2] < 128 <= values[3]


def test_change_point_counts():
    c = dc.case("change_points")
    lays = dc.layouts("change_points", True)
    assert set(c.marks["at"]) | {0} == set(dc.CP_COUNTS)
    for n, p in c.marks["at"].items():
        assert lays[0]["ncp"][p] == n, (n, p)
    seen = set(np.unique(lays[0]["ncp"]).tolist())
    assert set(dc.CP_COUNTS) <= seen and {dc.INLINE_CPS, dc.INLINE_CPS + 1} <= seen
    # 252 is what one position can be given: the copies of 3 .. 254 bytes, each with the byte that ends it, reach
    # 32 634 positions back and the next one would leave the window
    assert sum(l + 1 for l in dc.MAX_CPS) < 32768 <= sum(l + 1 for l in dc.MAX_CPS + [dc.MAX_CPS[-1] + 1])
    for key, pool in (("cut_pool", True), ("cut_inline", False)):
        b, j, planted = c.marks[key]
        lay = lays[b]
        B = len(lay["kend"])
        assert B - j <= 258 and lay["kend"][j] == lay["length"][j] == B - j          # the block end cuts the row
        assert (lay["ncp"][j] > dc.INLINE_CPS) == pool and 7 <= lay["ncp"][j] < planted   # ... through its change points


def test_subchunk_totals():
    c = dc.case("subchunks")
    lay = dc.layouts("subchunks", True)[0]
    chunks = dc.subchunks(lay)
    by_first = {q: (q, n, tot) for q, n, tot in chunks}
    want = c.marks["want"]
    assert [x for x in chunks if 384 <= x[0] < 448] == want[384]                      # 64 rows of 258 slots
    assert np.all(lay["lay"][384:448] == 258)
    assert by_first[640] == want[640] and lay["lay"][647] == 253 and want[640][2] + 253 == dc.EG_CAP + 1   # pushed on
    assert by_first[1344] == want[1344] and want[1344][2] == dc.EG_CAP
    assert by_first[2368] == want[2368] and want[2368][2] == dc.EG_CAP - 1 and lay["lay"][2368 + 59] == 258
    assert sum(n for _, n, _ in chunks) == len(lay["lay"]) and sum(t for _, _, t in chunks) == lay["block_edges"]
    # records of more than 8 change points: first row of a sub-chunk, last row, two in one
    pool = np.flatnonzero(lay["ncp"] > dc.INLINE_CPS)
    assert set(c.marks["pool"]) <= set(pool.tolist())
    firsts = {q for q, _, _ in chunks}
    lasts = {q + n - 1 for q, n, _ in chunks}
    assert c.marks["pool"][0] in firsts and c.marks["pool"][1] in lasts
    assert any(sum(q <= p < q + n for p in pool) >= 2 for q, n, _ in chunks)


def test_symbols_covered():
    lay = dc.layouts("symbols", True)[0]
    lits = lay["codes"][lay["roff"][lay["codeless"] == 0]]
    assert set((lits // 8 - 1).tolist()) == set(range(256))
    assert set(lay["edge_len"][lay["edge_len"] > 0].tolist()) == set(range(3, 259))
    dists = set(lay["edge_dist"].tolist())
    bounds = dc.dist_boundaries()
    assert set(bounds) <= dists, sorted(set(bounds) - dists)
    assert len(bounds) == 4 + 2 * 26 and bounds[0] == 1 and bounds[-1] == 32767
    syms = set(((lay["codes"][lay["edge_len"] > 0].astype(np.int64) // 8 - 257) % 30).tolist())
    assert syms == set(range(30))


def test_shortcut_flag_flips():
    c = dc.case("shortcut")
    lays = dc.layouts("shortcut", True)
    for what, (b, j, flipped) in c.marks["flips"].items():
        lay = lays[b]
        B = len(lay["kend"])
        assert lay["shortcut"][j] != lay["shortcut"][j + 1], what
        hold = [(int(lay["same"][q]) > 516, q > 259, q + 517 < B, int(lay["same"][q - 258]) > 258) for q in (j, j + 1)]
        # one inequality flips between the neighbours and the other three hold — but for the block end, where same[]
        # (counted inside the block, hash.c:116-126) falls to 516 at the very position at which j + 517 reaches B
        assert [i for i in range(4) if hold[0][i] != hold[1][i]] == flipped, (what, hold)
        assert all(hold[0][i] and hold[1][i] for i in range(4) if i not in flipped), (what, hold)
    big = lays[1]
    at = np.flatnonzero(big["shortcut"])
    assert len(at) > 65000
    assert big["same"][at[0]] == 65535 and big["same"][at[0] - 258] == 65535          # saturated on both sides
    assert big["same"][at[-1]] == 517 and not big["shortcut"][at[-1] + 1]


def test_rows_that_are_no_run_rows():
    c = dc.case("not_run_rows")
    lay = dc.layouts("not_run_rows", True)[0]
    p = c.marks["far"]
    assert lay["same"][p] > 0 and lay["ncp"][p] == 2 and lay["dist"][p] == 200 and not lay["run_row"][p]
    assert lay["edge_dist"][lay["roff"][p] + 2] == 1                                   # its first change point is the run's
    r = c.marks["run66"]
    assert lay["kend"][r + 1:r + 5].tolist() == [65, 64, 63, 62] and np.all(lay["run_row"][r + 1:r + 5] == 1)
    assert lay["codeless"][r + 1:r + 5].tolist() == [1, 1, 0, 0]


def test_window_kinds():
    kinds, mixed_wave, partial_clean, cross = set(), 0, 0, {64: 0, 128: 0}
    for name in dc.CASES:
        for lay in dc.layouts(name, True):
            B = len(lay["kend"])
            if B == 0:
                continue
            flag = lay["winflag"][:-1]
            kinds |= set((flag & 0xff).tolist()) | set((flag & dc.WF_CODELESS).tolist())
            assert lay["winflag"][-1] == 0 and lay["winroff"][-1] == lay["block_edges"]
            mixed_wave += int(np.count_nonzero(flag[0:len(flag) - 1:2] != flag[1::2]))
            full = B // 32
            reach = (lay["kend"].astype(np.int64) + np.arange(B) % 32)[:32 * full].reshape(full, 32)
            plain = (flag[:full] & 0xff) != 0                    # no shortcut flag, no wide run row: the reach alone decides
            cross[64] += int(np.count_nonzero(plain & (reach < 64).any(1) & (reach >= 64).any(1) & (reach < 128).all(1)))
            cross[128] += int(np.count_nonzero(plain & (reach < 128).any(1) & (reach >= 128).any(1)))
            if B % 32:
                tail = slice(B - B % 32, B)
                u = np.arange(B % 32)
                if not lay["shortcut"][tail].any() and np.all(lay["kend"][tail] + u < 64):
                    partial_clean += 1
                    assert flag[-1] & 0xff == 0         # full, it would be kind 1
    assert kinds == {0, 1, 2, 3, dc.WF_CODELESS}
    assert mixed_wave > 10 and partial_clean > 3
    assert cross[64] > 10 and cross[128] > 10, cross            # kend + u crosses 64 / 128 inside a window
