"""The synthetic block-cost cases (blockcost_cases.py) on the CPU: the host's CalculateBlockSizeAutoType (host/block_cost.cc)
and the ZopfliCalculateBlockSizeAutoType that libzopfli_amd.so exports equal the REAL reference on every generated range,
empty ranges included — integer equality of the returned doubles — and the generated inputs provably reach the decisions
they were built for (the coverage facts, asserted with the reference's own exported functions only).  The same cases price
k_block_cost in test_gpu_block_cost_synthetic.py.  CPU only."""
import ctypes

import numpy as np
import pytest

import blockcost_cases as bc
import oracle_lib as ol

pytestmark = pytest.mark.skipif(not ol.have_ref(), reason="oracle/_ref not built (needs the reference's sources)")

_u16p, _sz = ctypes.POINTER(ctypes.c_uint16), ctypes.c_size_t
FAMILY_NAMES = ("fibonacci", "powers", "all_used", "degenerate", "every_value", "uniform", "switch", "repeat_splits", "plateaus")
ZMX_ERR_REFUSED = 3


def _families(name):
    return [f for f in bc.all_families() if f.family == name]


def _ref_block_size():
    r = ol.ref()
    r.ZopfliCalculateBlockSize.argtypes = [ctypes.c_void_p, _sz, _sz, ctypes.c_int]
    r.ZopfliCalculateBlockSize.restype = ctypes.c_double
    return r


def test_generator_covers_the_families():
    """Every family of the list is generated, in both orders, below the limit, and a sequence has the histogram it was
    built from."""
    fams = bc.all_families()
    assert {f.family for f in fams} == set(FAMILY_NAMES)
    assert sum(f.family == "plateaus" for f in fams) >= 40
    assert len({repr(f) for f in fams}) == len(fams)
    for f in fams:
        assert 0 < f.size < bc.LIMIT
        if f.size > 300000:
            continue
        want = None
        for order in bc.ORDERS:
            ll, dd = f.sequence(order)
            assert len(ll) == len(dd) == f.size
            h = bc.histogram(ll, dd)
            assert np.array_equal(h[0][:256], f.lit), (f, order)
            assert h[0][257:286].sum() == h[1].sum()
            if want is not None:
                assert np.array_equal(h[0], want[0]) and np.array_equal(h[1], want[1]), f
            want = h
    # (the tables against oracle_lib's: two statements of RFC 1951 3.2.5)
    assert [int(s) for s in bc.length_symbols(list(range(3, 259)))] == [ol.length_symbol(l) for l in range(3, 259)]
    ds = list(range(1, 600)) + list(range(32000, 32769)) + bc.DIST_BASE
    assert [int(s) for s in bc.dist_symbols(ds)] == [ol.dist_symbol(d) for d in ds]


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_host_block_size_vs_reference(family):
    """zamd_test_block_size_auto (host/block_cost.cc) and the exported ZopfliCalculateBlockSizeAutoType of libzopfli_amd.so
    (on the reference's own store) == the reference's ZopfliCalculateBlockSizeAutoType, range by range, a == b included."""
    from zopfli_amd import api
    host = ol.hosttest_library()
    host.zamd_test_block_size_auto.argtypes = [_u16p, _u16p, _sz, _sz, _sz]
    host.zamd_test_block_size_auto.restype = ctypes.c_double
    mine = api.library()
    mine.ZopfliCalculateBlockSizeAutoType.argtypes = [ctypes.c_void_p, _sz, _sz]
    mine.ZopfliCalculateBlockSizeAutoType.restype = ctypes.c_double
    checked = 0
    for i, f in enumerate(_families(family)):
        for order in bc.ORDERS:
            ll, dd = f.sequence(order)
            rs = ol.RefSymbols(ll, dd)
            try:
                p = ctypes.addressof(rs.store)
                pl, pd = ll.ctypes.data_as(_u16p), dd.ctypes.data_as(_u16p)
                for a, b in bc.ranges(f.size, seed=i):
                    want = rs.block_size_auto(a, b)
                    assert float(want).is_integer()
                    if a == b:
                        assert want == 0.0, (f, order, a, b)
                    got = host.zamd_test_block_size_auto(pl, pd, f.size, a, b)
                    assert got == want, f"host block_cost.cc: {f} {order} [{a}, {b}): {got} != {want}"
                    got = mine.ZopfliCalculateBlockSizeAutoType(p, a, b)
                    assert got == want, f"exported AutoType: {f} {order} [{a}, {b}): {got} != {want}"
                    checked += 1
            finally:
                rs.close()
    assert checked > 0


# ---- coverage facts: about the INPUTS, by the reference's exported functions only
def _whole_counts(f):
    """the whole sequence's counts as GetDynamicLengths sees them: the end symbol counted once (deflate.c:577)"""
    ll, dd = f.sequence("sorted")
    h_ll, h_d = bc.histogram(ll, dd)
    h_ll[256] = 1
    return h_ll, h_d


def _ref_smoothed(counts):
    """OptimizeHuffmanForRle (deflate.c:434) of a copy"""
    n = len(counts)
    arr = (_sz * n)(*[int(c) for c in counts])
    ol.ref().OptimizeHuffmanForRle.argtypes = [ctypes.c_int, ctypes.POINTER(_sz)]
    ol.ref().OptimizeHuffmanForRle.restype = None
    ol.ref().OptimizeHuffmanForRle(n, arr)
    return np.asarray(list(arr), dtype=np.int64)


def _ref_lengths(counts):
    rc, lengths = ol.ref_code_lengths(counts, 15)
    assert rc == 0
    return lengths


def test_coverage_length_limit():
    """ZopfliLengthLimitedCodeLengths reaches length 15 on the litlen alphabet of one case and on the distance alphabet of
    one case."""
    hit_ll, hit_d = [], []
    for f in bc.families():
        h_ll, h_d = _whole_counts(f)
        if max(_ref_lengths(h_ll)) == 15:
            hit_ll.append(repr(f))
        if max(_ref_lengths(h_d)) == 15:
            hit_d.append(repr(f))
    assert hit_ll and hit_d, (hit_ll, hit_d)


def test_coverage_block_types():
    """Each of stored, fixed and dynamic is the strict minimum of ZopfliCalculateBlockSize(..., btype) on an asked range."""
    r = _ref_block_size()
    winners = {0: None, 1: None, 2: None}
    for name in ("uniform", "switch", "degenerate", "every_value"):
        for i, f in enumerate(_families(name)):
            ll, dd = f.sequence("shuffled")
            rs = ol.RefSymbols(ll, dd)
            try:
                p = ctypes.addressof(rs.store)
                for a, b in bc.ranges(f.size, seed=i):
                    if a == b:
                        continue
                    c = [r.ZopfliCalculateBlockSize(p, a, b, t) for t in (0, 1, 2)]
                    t = int(np.argmin(c))
                    if sorted(c)[0] < sorted(c)[1] and winners[t] is None:
                        winners[t] = (repr(f), a, b, c)
            finally:
                rs.close()
    assert all(w is not None for w in winners.values()), winners
    # ... and the fixed tree wins inside a store of at most 1000 symbols, where AutoType may take it (deflate.c:615)
    f = [x for x in _families("switch") if x.name == "n1000"][0]
    ll, dd = f.sequence("shuffled")
    rs = ol.RefSymbols(ll, dd)
    try:
        p = ctypes.addressof(rs.store)
        fixed_wins = [(a, b) for a, b in bc.ranges(f.size, seed=0) if a < b and
                      r.ZopfliCalculateBlockSize(p, a, b, 1) < min(r.ZopfliCalculateBlockSize(p, a, b, 0), r.ZopfliCalculateBlockSize(p, a, b, 2))]
        assert fixed_wins
    finally:
        rs.close()


def test_coverage_smoothing_changes_the_plateaus():
    """OptimizeHuffmanForRle changes the counts of at least half of the plateau draws."""
    draws = _families("plateaus")
    changed = 0
    for f in draws:
        h_ll, h_d = _whole_counts(f)
        if not (np.array_equal(_ref_smoothed(h_ll), h_ll) and np.array_equal(_ref_smoothed(h_d), h_d)):
            changed += 1
    print(f"OptimizeHuffmanForRle changes {changed} of {len(draws)} plateau draws")
    assert 2 * changed >= len(draws), (changed, len(draws))


def _header_runs(ll_lengths, d_lengths):
    """run lengths of equal code lengths in ll_lengths ++ d_lengths as the tree header sends them: two distance codes at
    least (deflate.c:86-103), trailing zeros beyond hlit / hdist dropped (deflate.c:122-123)"""
    d = list(d_lengths[:30])
    used = [i for i in range(30) if d[i]]
    if len(used) == 0:
        d[0] = d[1] = 1
    elif len(used) == 1:
        d[1 if used[0] == 0 else 0] = 1
    hlit = max([i + 1 for i in range(29) if ll_lengths[257 + i]], default=0)
    hdist = max([i for i in range(1, 30) if d[i]], default=0)
    seq = list(ll_lengths[:257 + hlit]) + d[:hdist + 1]
    zero, nonzero = set(), set()
    i = 0
    while i < len(seq):
        j = i
        while j < len(seq) and seq[j] == seq[i]:
            j += 1
        (zero if seq[i] == 0 else nonzero).add(j - i)
        i = j
    return zero, nonzero


def test_coverage_repeat_code_split_points():
    """The runs of equal code lengths (the reference's lengths of the whole-range histograms, as they are and smoothed) hold
    zero runs of exactly 2, 3, 10, 11, 138 and >= 139 and non-zero runs of exactly 3, 4, 6, 7 and >= 8: the split points of the
    repeat codes 16 / 17 / 18."""
    zero, nonzero = set(), set()
    for f in bc.all_families():
        h_ll, h_d = _whole_counts(f)
        for c_ll, c_d in ((h_ll, h_d), (_ref_smoothed(h_ll), _ref_smoothed(h_d))):
            z, nz = _header_runs(_ref_lengths(c_ll), _ref_lengths(c_d))
            zero |= z
            nonzero |= nz
    assert {2, 3, 10, 11, 138} <= zero and max(zero) >= 139, sorted(zero)
    assert {3, 4, 6, 7} <= nonzero and max(nonzero) >= 8, sorted(nonzero)


# ---- the refusals of zmx_cost_stores_create_host, by the oracle backend's copy of the device layer's check
INVALID_SYMBOLS = [(256, 0), (300, 0), (40000, 0), (2, 5), (259, 5), (100, 32769), (100, 65535)]


@pytest.mark.parametrize("litlen,dist", INVALID_SYMBOLS)
def test_invalid_symbols_are_refused_host_backend(litlen, dist):
    """A pair that is no LZ77 symbol (host/symbol_check.h) is refused with ZMX_ERR_REFUSED wherever it stands; the context
    prices a valid sequence afterwards."""
    from zopfli_amd import Context, api
    host = ol.hosttest_library()
    ctx = Context(0, host)
    try:
        good = bc.all_families()[0].sequence("shuffled")
        for at in (0, 7, len(good[0]) - 1):
            ll, dd = good[0].copy(), good[1].copy()
            ll[at], dd[at] = litlen, dist
            with pytest.raises(RuntimeError, match="no LZ77 symbol"):
                api.CostStores.from_host(ctx, [good, (ll, dd)])
            assert host.zmx_last_error_class() == ZMX_ERR_REFUSED
        cs = api.CostStores.from_host(ctx, [good])
        try:
            rs = ol.RefSymbols(*good)
            try:
                assert cs.block_costs([(0, 0, len(good[0]))])[0] == rs.block_size_auto(0, len(good[0]))
            finally:
                rs.close()
        finally:
            cs.free()
    finally:
        ctx.close()


def test_valid_symbol_edges_are_accepted_host_backend():
    """The rule's edges on the valid side: literals 0 and 255, lengths 3 and 258, distances 1 and 32768."""
    from zopfli_amd import Context, api
    host = ol.hosttest_library()
    ctx = Context(0, host)
    try:
        ll = np.array([0, 255, 3, 258, 3, 258], dtype=np.uint16)
        dd = np.array([0, 0, 1, 1, 32768, 32768], dtype=np.uint16)
        cs = api.CostStores.from_host(ctx, [(ll, dd)])
        rs = ol.RefSymbols(ll, dd)
        try:
            assert cs.block_costs([(0, 0, 6)])[0] == rs.block_size_auto(0, 6)
        finally:
            rs.close()
            cs.free()
    finally:
        ctx.close()


@pytest.mark.parametrize("cls", ["B", "T"])
def test_glued_stores_host_backend(cls):
    """The oracle backend's zmx_cost_stores_create — whole stores, strict prefixes, blocks out of order, the two slots
    mixed — prices like the reference prices the same symbols (the body of the GPU file's test_device_stores_vs_reference):
    a sequence counts its own bytes, wherever its pieces lie in the input."""
    from test_gpu_block_cost_synthetic import device_stores_vs_reference
    from zopfli_amd import Context
    ctx = Context(0, ol.hosttest_library())
    try:
        device_stores_vs_reference(ctx, cls)
    finally:
        ctx.close()
