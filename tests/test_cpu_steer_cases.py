"""What the steered inputs of steer_cases.py reach, asserted with the CPU oracle and plain Python alone — the GPU files
(test_gpu_mincost_edges.py, test_gpu_bit_writer_limits.py, test_gpu_verify_reports.py) hold the kernels to the same
references, so a case that stopped reaching its path would fail HERE, without a GPU.  CPU only."""
import numpy as np
import pytest

import oracle_lib as ol
import seg_probe
import steer_cases as sc
from test_gpu_parity import _fixed_codes, _py_symbol_bits


# ------------------------------------------------------------------------------------------------ sub-mincost edges
@pytest.mark.parametrize("name", [c[0] for c in sc.INFLATED])
def test_inflated_mincost_changes_the_parse(name):
    """mincost = GetCostModelMinCost + delta: match weights lie below it (which ones follows from the model alone), and
    the oracle's length array differs from the one for the true mincost — a kernel that ignored squeeze.c:293's test
    would be caught by these cases.  Measured (weights below, positions that differ): T delta 1: 13, 42; T delta 3: 180,
    3580; B delta 0.25: 4, 231; P delta 3 with a window before the block: 140, 2664; Z delta 10 in two blocks: 27 each
    (16 or more of them length symbols at distance symbol 0), 1729 and 816; M delta 3: 434 and 1986 in the two blocks of
    real size, none in the blocks of 0 to 3 bytes."""
    c = sc.inflated(name)
    for b, (s, e) in enumerate(c["blocks"]):
        ll, d = c["cost"][b, :288], c["cost"][b, 288:]
        assert c["mincost_true"][b] == ol.model_min_cost(ll, d)
        assert sc.weights_below(ll, d, c["mincost_true"][b]) == []          # entropy costs: none below the true mincost
        below = sc.weights_below(ll, d, c["mincost"][b])
        assert len(below) > 0, (name, b)
        if name.startswith("Z"):
            # long runs are rows of (k, distance 1): k_badscan's branch for rows without codes looks up exactly these
            assert sum(1 for ls, ds in below if ds == 0) >= 16, below
    diff = sc.differing_positions(c["runs"], c["runs_true"])
    print(name, "weights below:", [len(sc.weights_below(c["cost"][b, :288], c["cost"][b, 288:], c["mincost"][b]))
                                   for b in range(len(c["blocks"]))], "positions that differ:", diff)
    total = sum(diff)
    assert total > 0, (name, diff)
    big = [b for b, (s, e) in enumerate(c["blocks"]) if e - s >= 30000]
    assert all(diff[b] > 0 for b in big), (name, diff)                      # every block of real size is reached


@pytest.mark.parametrize("name", [c[0] for c in sc.ROUNDING])
def test_rounding_model_has_a_weight_below_its_own_mincost(name):
    """mincost IS GetCostModelMinCost (1.25) and the weight of (length 4, distance 2) is 1.25 - 2^-52: inside the
    documented contract of zmx_squeeze_run, k_wtab still finds a weight below mincost.  The oracle's parse equals its
    parse for mincost 0 here, so the GPU leg on these models pins the flagged positions' generic path only."""
    c = sc.rounding(name)
    for b in range(len(c["blocks"])):
        ll, d = c["cost"][b, :288], c["cost"][b, 288:]
        assert c["mincost"][b] == ol.model_min_cost(ll, d) == 1.25
        assert (258, 1) in sc.weights_below(ll, d, c["mincost"][b])
        assert (float(0 + 0) + ll[258]) + d[1] == 1.25 - 2.0 ** -52
    for a, z in zip(c["runs"], c["runs_zero"]):
        assert np.array_equal(a[0], z[0])
    # the weight is used: matches of length 4 at distance 2 occur in the parse of the two-symbol class
    if name == "B":
        assert any(np.any((r[1] == 4) & (r[2] == 2)) for r in c["runs"])


def test_state_runs_alternate_clean_and_bad():
    """The run sequence of test_gpu_mincost_edges.test_state_across_runs: clean, bad, clean, bad in ONE block of three,
    clean — the bad runs differ from the clean ones exactly in the blocks whose mincost was raised."""
    c = sc.state_runs()
    clean = c["runs"][0][1]
    for (dl, (mincost, runs)) in zip(sc.STATE_RUNS, c["runs"]):
        diff = sc.differing_positions(runs, clean)
        for b, x in enumerate(dl):
            ll, d = c["cost"][b, :288], c["cost"][b, 288:]
            assert (len(sc.weights_below(ll, d, mincost[b])) > 0) == (x > 0)
            assert (diff[b] > 0) == (x > 0), (dl, diff)


def test_probe_mincost_cases_reach():
    """seg_probe.py's SEG_PROBE_MINCOST cases (class T and class Z, at most 200 KB): the first inflated run of each
    differs from the true-mincost run of the oracle."""
    for cls, n, blocks, delta in seg_probe.mincost_cases(3.0):
        assert n <= 200000
        data = sc.generate(cls, n)
        cost, true = sc.cost_rows([ol.entropy_costs(h) for h in sc.greedy_hists(data, blocks)])
        diff = sc.differing_positions(sc.oracle_run(data, blocks, cost, true + delta), sc.oracle_run(data, blocks, cost, true))
        print(cls, delta, diff)
        assert all(x > 0 for x in diff), (cls, diff)
        if cls == "Z":
            assert delta >= 10 and all(sum(1 for ls, ds in sc.weights_below(cost[b, :288], cost[b, 288:], true[b] + delta)
                                           if ds == 0) > 0 for b in range(len(blocks)))


# ------------------------------------------------------------------------------------------------ steered stores
def test_all_literal_stores_have_exact_sizes():
    """Exact tile multiples (the last tile of the bit writer holds the end symbol alone), one symbol either side, and
    more than 64 tiles (k_enc_scan's loop goes round twice)."""
    c = sc.steered("literals")
    sizes = [len(r[1]) for r in c["runs"]]
    assert sizes == [2047, 2048, 2049, 4096, 64 * sc.ENC_TILE + 1]
    for (s, e), (la, ll, dd) in zip(c["blocks"], c["runs"]):
        assert not dd.any() and ll.tobytes() == np.frombuffer(c["data"][s:e], dtype=np.uint8).astype(np.uint16).tobytes()
    assert sizes[1] % sc.ENC_TILE == 0 and sizes[3] % sc.ENC_TILE == 0
    assert sizes[4] // sc.ENC_TILE + 1 == 65 > 64
    assert np.all(c["cost"] >= 0) and np.all(c["cost"] <= 24)


def test_tile48_store_fills_a_tile():
    """2068 or more consecutive symbols of 48 bits under 15-bit codes: a full tile of 2048 * 48 = 98304 bits (all of
    the tile's bit buffer) with a partial tile behind it."""
    c = sc.steered("tile48")
    (la, ll, dd), = c["runs"]
    assert len(ll) >= 2068
    assert np.all(dd == 20000) and ll.min() >= 131 and ll.max() <= 257
    bits = sc.symbol_bits(ll, dd, sc.codes_15bit(1))
    assert sc.longest_run_of(bits, 48) >= 2068
    _, total = sc.tile_starts(bits)
    assert total[0] == sc.ENC_TILE * 48 and 0 < total[1] < sc.ENC_TILE * 48
    assert np.all(c["cost"] >= 0) and np.all(c["cost"] <= 24)


def test_tile48_mixed_hits_every_third_word_shift():
    """The literal-mixed variant: a symbol that needs the third 32-bit word of the tile buffer (sh + n > 64) occurs at
    every shift sh = 17 .. 31, and prefixes of the store exist whose end symbol (15 bits) crosses a word at every
    shift 18 .. 31 (test_gpu_bit_writer_limits takes such prefixes as jobs)."""
    c = sc.steered("tile48_mixed")
    (la, ll, dd), = c["runs"]
    bits = sc.symbol_bits(ll, dd, sc.codes_15bit(1))
    assert np.count_nonzero(dd == 0) > 100 and np.count_nonzero(bits == 48) > 1000
    assert sc.three_word_shifts(bits) >= set(range(17, 32))
    ends = sc.end_symbol_prefixes(bits)
    assert set(ends) == set(range(18, 32))
    for sh, n in ends.items():
        _, total = sc.tile_starts(bits[:n])
        assert total[-1] & 31 == sh and sh + 15 > 32


def test_tile_writer_equals_the_plain_writer():
    """steer_cases.write_symbols (the Python writer applied tile by tile) == the writer applied once, on stores around
    the tile size, with the fixed tree and with 15-bit codes, at several bit offsets."""
    c = sc.steered("literals")
    m = sc.steered("tile48_mixed")["runs"][0]
    fixed = _fixed_codes()[0]
    for ll, dd in [c["runs"][0][1:], c["runs"][1][1:], c["runs"][2][1:], c["runs"][3][1:], (m[1][:5000], m[2][:5000])]:
        for codes, start in ((fixed, 0), (sc.codes_15bit(7), 3), (sc.codes_mixed(8), 77), (sc.codes_sparse(ll, dd, 9), 4100)):
            want = _py_symbol_bits(ll, dd, codes, start)
            assert sc.write_symbols(_py_symbol_bits, ll, dd, codes, start) == want
            assert want[1] == int(sc.symbol_bits(ll, dd, codes).sum()) + (int(codes[256]) >> 16)


def test_code_tables():
    assert np.all(sc.codes_15bit(3) >> 16 == 15)
    assert set((sc.codes_mixed(3) >> 16).tolist()) == set(range(1, 16))
    ll, dd = sc.steered("tile48_mixed")["runs"][0][1:]
    sp = sc.codes_sparse(ll, dd, 3)
    ls, ds = sc.symbols_of(ll, dd)
    assert np.count_nonzero(sp == 0) > 20 and np.all(sp[ls] >> 16 > 0) and np.all(sp[288 + ds[ds >= 0]] >> 16 > 0) and sp[256] >> 16 > 0
    for t in (sc.codes_15bit(3), sc.codes_mixed(3), sp):
        assert np.all((t & 0xffff) < (1 << (t >> 16)))


# ------------------------------------------------------------------------------------------------ verify reference
def test_python_verify_names_the_first_failure():
    """steer_cases.verify_len_dist (ZopfliVerifyLenDist, lz77.c:270-295, over a whole store) on a hand-made store."""
    data = b"abcabcabcxyz"
    ll = np.array([97, 98, 99, 6, 120, 121, 122], dtype=np.uint16)
    dd = np.array([0, 0, 0, 3, 0, 0, 0], dtype=np.uint16)
    assert sc.verify_len_dist(data, 0, len(data), ll, dd) is None
    assert sc.verify_len_dist(data, 0, len(data), ll[:-1], dd[:-1]) == (6, 3)
    assert sc.verify_len_dist(b"abcabcabQxyz", 0, 12, ll, dd) == (3, 2)
    assert sc.verify_len_dist(b"abcabcabQxyZ", 0, 12, ll, dd) == (3, 2)
    assert sc.verify_len_dist(b"Xbcabcabcxyz", 0, 12, ll, dd) == (0, 2)
    assert sc.verify_len_dist(data, 0, 12, np.array([97, 98, 99, 259], dtype=np.uint16), np.array([0, 0, 0, 3], dtype=np.uint16)) == (3, 1)
