"""k_block_cost (csrc/device/zmx_blockcost.h) against the REAL reference's ZopfliCalculateBlockSizeAutoType
(deflate.c:610-621) on histograms built to reach what the kernel re-derives — the level-by-level package-merge and its tie
rule, the eight tree headers side by side, the smoothing's frozen runs and thresholds, the sampled prefix counts — and on
the edges of the entry points: many sequences in one object, sequences glued from device stores, the 2^22 limit and pairs
that are no LZ77 symbols.  Every comparison is integer equality of the returned doubles; the cases are those of
blockcost_cases.py, whose reach test_cpu_block_cost_synthetic.py asserts."""
import numpy as np
import pytest

import blockcost_cases as bc
import oracle_lib as ol
from zopfli_amd import api, generate

pytestmark = pytest.mark.gpu

FAMILY_NAMES = ("fibonacci", "powers", "all_used", "degenerate", "every_value", "uniform", "switch", "repeat_splits", "plateaus")
ZMX_ERR_REFUSED = 3


def _need_ref():
    assert ol.have_ref(), "oracle/_ref/libzopfli_ref.so not built"


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_families_vs_reference(gpu_ctx, family):
    """Every family in both orders: whole sequences, single symbols, empty ranges, ends on and beside the samples, widths
    around the direct-count threshold, random ranges."""
    _need_ref()
    fams = [f for f in bc.all_families() if f.family == family]
    assert fams
    for i, f in enumerate(fams):
        for order in bc.ORDERS:
            ll, dd = f.sequence(order)
            rs = ol.RefSymbols(ll, dd)
            cs = api.CostStores.from_host(gpu_ctx, [(ll, dd)])
            try:
                rg = bc.ranges(f.size, seed=i)
                got = cs.block_costs([(0, a, b) for a, b in rg])
                for (a, b), g in zip(rg, got.tolist()):
                    want = rs.block_size_auto(a, b)
                    assert g == want, f"{f} {order} [{a}, {b}): device {g}, reference {want}"
            finally:
                cs.free()
                rs.close()


def _random_sequence(rng, n):
    nlit = int(rng.integers(1, 257))
    base = int(rng.integers(0, 256 - nlit + 1))
    p = rng.random(nlit) ** int(rng.integers(1, 6))
    lits = base + rng.choice(nlit, n, p=p / p.sum())
    is_match = rng.random(n) < float(rng.choice([0.0, 0.05, 0.3, 0.9]))
    lens = np.where(rng.random(n) < 0.5, rng.integers(3, 259, n), rng.integers(3, 12, n))
    dists = np.clip((2.0 ** (rng.random(n) * 15.0)).astype(np.int64), 1, 32768)
    return np.where(is_match, lens, lits).astype(np.uint16), np.where(is_match, dists, 0).astype(np.uint16)


def test_many_sequences_in_one_object(gpu_ctx):
    """320 sequences of one zmx_cost_stores — empty, one symbol, around the 1000-symbol switch, around the samples — their
    ranges interleaved in one call, a small call before the large one (the evaluation buffers grow), and
    zmx_cost_positions against the running sum of the symbols' spans."""
    _need_ref()
    rng = np.random.default_rng(22)
    sizes = [0, 1, 2, 1000, 1001, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096]
    sizes += rng.integers(0, 6000, 320 - len(sizes)).tolist()
    order = rng.permutation(len(sizes))
    seqs = [_random_sequence(rng, int(sizes[k])) for k in order]
    refs = [ol.RefSymbols(ll, dd) for ll, dd in seqs]
    cs = api.CostStores.from_host(gpu_ctx, seqs)
    try:
        assert cs.sizes == [len(s[0]) for s in seqs]
        ranges = [(q, a, b) for q, s in enumerate(seqs) for a, b in bc.ranges(len(s[0]), seed=q, nrandom=2)]
        ranges = [ranges[k] for k in rng.permutation(len(ranges))]
        for part in (ranges[:40], ranges):
            got = cs.block_costs(part)
            for (q, a, b), g in zip(part, got.tolist()):
                want = refs[q].block_size_auto(a, b)
                assert g == want, f"sequence {q} of {len(seqs[q][0])} symbols [{a}, {b}): device {g}, reference {want}"
        pairs, want = [], []
        for q, (ll, dd) in enumerate(seqs):
            m = len(ll)
            csum = np.concatenate([[0], np.cumsum(np.where(dd == 0, 1, ll).astype(np.uint64))])
            idx = {0, 1, m}
            for k in range(1024, m + 2, 1024):
                idx |= {k - 1, k, k + 1}
            for i in sorted(x for x in idx if 0 <= x <= m):
                pairs.append((q, i))
                want.append(int(csum[i]))
        assert cs.positions(pairs).tolist() == want
    finally:
        cs.free()
        for r in refs:
            r.close()


def _valid_symbols(ll, dd):
    lit = dd == 0
    return bool(np.all(np.where(lit, ll <= 255, (ll >= 3) & (ll <= 258) & (dd <= 32768))))


def device_stores_vs_reference(gpu_ctx, cls):
    """(the body of test_device_stores_vs_reference; test_cpu_block_cost_synthetic.py runs it on the oracle backend too)"""
    n = 150000
    data = generate(cls, n, seed=31)
    gpu_ctx.set_input(data)
    blocks = [(0, 60000), (60000, 100000), (100000, n)]
    t = gpu_ctx.build_tables(blocks)
    refs, dev = [], None
    try:
        nsym0, hist = t.greedy(0)
        cost, mincost = np.zeros((3, 320)), np.zeros(3)
        for b in range(3):
            c_ll, c_d = ol.entropy_costs(hist[b])
            cost[b, :288], cost[b, 288:] = c_ll, c_d
            mincost[b] = ol.model_min_cost(c_ll, c_d)
        nsym1, _ = t.squeeze_run(cost, mincost, np.ones(3, dtype=np.int32))
        ns = [[int(x) for x in nsym0], [int(x) for x in nsym1]]
        assert all(k >= 4 for s in ns for k in s)
        sequences = []
        for s in (0, 1):
            sequences += [[(0, s, ns[s][0])],
                          [(b, s, ns[s][b]) for b in range(3)],
                          [(2, s, ns[s][2]), (0, s, ns[s][0]), (1, s, ns[s][1])],
                          [(1, s, ns[s][1] // 2)],
                          [(0, s, ns[s][0] - 1), (2, s, 1), (1, s, ns[s][1] // 3)]]
        sequences += [[(0, 1, ns[1][0]), (1, 0, ns[0][1]), (2, 1, ns[1][2] - 1)]]
        dev = api.CostStores.from_tables(t, sequences)
        ranges = []
        for q, seq in enumerate(sequences):
            parts = [t.store(b, s, k) for b, s, k in seq]
            ll, dd = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
            assert _valid_symbols(ll, dd), f"{cls}: sequence {q} downloads pairs that are no symbols"
            assert dev.sizes[q] == len(ll)
            refs.append(ol.RefSymbols(ll, dd))
            ranges += [(q, a, b) for a, b in bc.ranges(len(ll), seed=q, nrandom=6)]
        got = dev.block_costs(ranges)
        for (q, a, b), g in zip(ranges, got.tolist()):
            want = refs[q].block_size_auto(a, b)
            assert g == want, f"{cls}: sequence {sequences[q]} [{a}, {b}): device {g}, reference {want}"
    finally:
        if dev is not None:
            dev.free()
        for r in refs:
            r.close()
        t.free()


@pytest.mark.parametrize("cls", ["Z", "B", "T"])
def test_device_stores_vs_reference(gpu_ctx, cls):
    """zmx_cost_stores_create: sequences glued from the device's own stores — the greedy store (slot 0) and an optimal parse
    (slot 1, one squeeze run with entropy costs): whole stores, strict prefixes of stores, three blocks out of order, the two
    slots mixed — price like the REFERENCE prices the same symbols, downloaded with Tables.store."""
    _need_ref()
    device_stores_vs_reference(gpu_ctx, cls)


def _prices_a_normal_sequence(gpu_ctx):
    ll, dd = bc.families()[0].sequence("shuffled")
    rs = ol.RefSymbols(ll, dd)
    cs = api.CostStores.from_host(gpu_ctx, [(ll, dd)])
    try:
        assert cs.block_costs([(0, 0, len(ll))])[0] == rs.block_size_auto(0, len(ll))
    finally:
        cs.free()
        rs.close()


def test_sequence_limit(gpu_ctx, gpu_lib):
    """A sequence of 2^22 - 1 symbols is accepted and prices as the reference prices it; one of 2^22 symbols is refused
    (ZMX_ERR_REFUSED), and the context prices a normal sequence afterwards."""
    _need_ref()
    m = bc.LIMIT - 1
    ll, dd = bc.near_limit(m)
    rs = ol.RefSymbols(ll, dd)
    cs = api.CostStores.from_host(gpu_ctx, [(ll, dd)])
    try:
        rg = [(0, m), (1, m), (0, m - 1), (m // 2, m), (m - 2048, m), (m - 1, m)]
        got = cs.block_costs([(0, a, b) for a, b in rg])
        for (a, b), g in zip(rg, got.tolist()):
            want = rs.block_size_auto(a, b)
            assert g == want, f"2^22 - 1 symbols [{a}, {b}): device {g}, reference {want}"
    finally:
        cs.free()
        rs.close()
    with pytest.raises(RuntimeError, match="2\\^22"):
        api.CostStores.from_host(gpu_ctx, [bc.near_limit(bc.LIMIT)])
    assert gpu_lib.zmx_last_error_class() == ZMX_ERR_REFUSED
    _prices_a_normal_sequence(gpu_ctx)


INVALID_SYMBOLS = [(256, 0), (300, 0), (40000, 0), (2, 5), (259, 5), (100, 32769), (100, 65535)]


@pytest.mark.parametrize("litlen,dist", INVALID_SYMBOLS)
def test_invalid_symbols_are_refused(gpu_ctx, gpu_lib, litlen, dist):
    """A pair that is no LZ77 symbol — a literal above 255, a length outside 3 .. 258, a distance above 32768 — would index a
    wave's histogram out of place: zmx_cost_stores_create_host refuses it on the host (host/symbol_check.h, before any
    allocation or launch) with ZMX_ERR_REFUSED, wherever it stands, and the context prices a normal sequence afterwards."""
    _need_ref()
    good = bc.families()[0].sequence("shuffled")
    for at in (0, 7, len(good[0]) - 1):
        ll, dd = good[0].copy(), good[1].copy()
        ll[at], dd[at] = litlen, dist
        with pytest.raises(RuntimeError, match="no LZ77 symbol"):
            api.CostStores.from_host(gpu_ctx, [good, (ll, dd)])
        assert gpu_lib.zmx_last_error_class() == ZMX_ERR_REFUSED
    _prices_a_normal_sequence(gpu_ctx)
