"""Synthetic LZ77 symbol sequences for the block-cost tests (test_cpu_block_cost_synthetic.py,
test_gpu_block_cost_synthetic.py): sequences built FROM A TARGET HISTOGRAM — literal counts[256], length-symbol
counts[29], distance-symbol counts[30], the two match totals equal — so that the decisions of
ZopfliCalculateBlockSizeAutoType (deflate.c:610-621) that greedy parses of text and noise rarely reach are reached on
purpose: the 15-bit limit of the package-merge, ties at every level, the corners of the tree header (hlit, hdist, the
two distance codes, the repeat codes' split points), the thresholds of OptimizeHuffmanForRle and the 1000-symbol
fixed-tree switch.

Every sequence comes in two orders, symbol-sorted and shuffled with a fixed seed: prefix and suffix ranges of the two
see very different histograms.  Every sequence stays below 2^22 symbols (the library's limit, and the domain in which
the reference's sort comparator is defined: test_cpu_oracle_vs_reference.py, style 2).

Lengths and distances come from the base tables of RFC 1951 3.2.5, written out here."""
import numpy as np

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227,
            258]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577]
LIMIT = 1 << 22          # a sequence holds fewer symbols than this
ORDERS = ("sorted", "shuffled")

PLATEAU_RUNS = (1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 20, 70, 139, 140)
PLATEAU_VALUES = (0, 1, 2, 3, 5, 50, 1000)
PLATEAU_DRAWS = 48


def length_symbols(lengths):
    """257 + the index of the last base <= length (length 258 has symbol 285 to itself)."""
    return 256 + np.searchsorted(np.asarray(LEN_BASE), np.asarray(lengths), side="right")


def dist_symbols(dists):
    return np.searchsorted(np.asarray(DIST_BASE), np.asarray(dists), side="right") - 1


def histogram(litlens, dists):
    """ll_counts[288], d_counts[32] of a sequence, WITHOUT the end symbol (ZopfliLZ77GetHistogram, lz77.c:189-222)."""
    litlens, dists = np.asarray(litlens, dtype=np.int64), np.asarray(dists, dtype=np.int64)
    m = dists != 0
    ll = np.bincount(litlens[~m], minlength=288) + np.bincount(length_symbols(litlens[m]), minlength=288)
    d = np.bincount(dist_symbols(dists[m]), minlength=32)
    return ll[:288].astype(np.int64), d[:32].astype(np.int64)


class Family:
    """A target histogram (or, with `matches`, an explicit list of (length, distance) values next to the literal counts)."""

    def __init__(self, family, name, lit=None, ln=None, ds=None, matches=None):
        self.family, self.name = family, name
        self.lit = np.zeros(256, dtype=np.int64) if lit is None else np.asarray(lit, dtype=np.int64)
        assert self.lit.shape == (256,) and (self.lit >= 0).all()
        if matches is None:
            ln = np.zeros(29, dtype=np.int64) if ln is None else np.asarray(ln, dtype=np.int64)
            ds = np.zeros(30, dtype=np.int64) if ds is None else np.asarray(ds, dtype=np.int64)
            assert ln.shape == (29,) and ds.shape == (30,) and ln.sum() == ds.sum(), name
            self.lens = np.repeat(np.asarray(LEN_BASE), ln)
            self.dsts = np.repeat(np.asarray(DIST_BASE), ds)
        else:
            self.lens = np.asarray([l for l, _ in matches], dtype=np.int64)
            self.dsts = np.asarray([d for _, d in matches], dtype=np.int64)
        self.size = int(self.lit.sum()) + len(self.lens)
        assert 0 < self.size < LIMIT, (name, self.size)

    def sequence(self, order):
        """(litlens, dists) as uint16 arrays.  sorted: the literals ascending, then the matches by length (the distances
        ascending alongside).  shuffled: lengths and distances paired at random, all symbols permuted (a fixed seed)."""
        lits = np.repeat(np.arange(256), self.lit)
        lens, dsts = self.lens, self.dsts
        ll = np.concatenate([lits, lens])
        dd = np.concatenate([np.zeros(len(lits), dtype=np.int64), dsts])
        if order == "shuffled":
            rng = np.random.default_rng(0x5eed)
            dd[len(lits):] = rng.permutation(dsts)
            p = rng.permutation(len(ll))
            ll, dd = ll[p], dd[p]
        else:
            assert order == "sorted"
        return ll.astype(np.uint16), dd.astype(np.uint16)

    def __repr__(self):
        return f"{self.family}/{self.name}"


def _fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return np.asarray(f[:n], dtype=np.int64)


def _at(n, pairs):
    a = np.zeros(n, dtype=np.int64)
    for i, c in pairs:
        a[i] = c
    return a


def _spread(total, n):
    """`total` over n symbols, as evenly as it goes."""
    a = np.full(n, total // n, dtype=np.int64)
    a[:total % n] += 1
    return a


def _balance(rng, ln, ds):
    """equal match totals: the difference goes to one symbol of the lighter alphabet"""
    diff = int(ln.sum() - ds.sum())
    if diff > 0:
        ds[int(rng.integers(0, 30))] += diff
    elif diff < 0:
        ln[int(rng.integers(0, 29))] -= diff


def plateau_counts(rng, n):
    """runs of equal or +-3-jittered counts; 40% of the runs are zero"""
    out = []
    while len(out) < n:
        run = int(rng.choice(PLATEAU_RUNS))
        if rng.random() < 0.4:
            out += [0] * run
            continue
        v = int(rng.choice(PLATEAU_VALUES))
        jitter = rng.random() < 0.5
        out += [max(0, v + (int(rng.integers(-3, 4)) if jitter else 0)) for _ in range(run)]
    return np.asarray(out[:n], dtype=np.int64)


def plateau_family(draw):
    rng = np.random.default_rng(7000 + draw)
    ll = plateau_counts(rng, 286)
    lit, ln = ll[:256].copy(), ll[257:286].copy()
    ds = plateau_counts(rng, 30)
    _balance(rng, ln, ds)
    if lit.sum() + ln.sum() == 0:
        lit[0] = 1
    return Family("plateaus", f"draw{draw}", lit, ln, ds)


def _repeat_splits():
    """Counts 2^(9 - length) for a complete code, so the code lengths are forced: non-zero runs of exactly 3, 4, 6, 7 and 8
    equal lengths, between zero runs of exactly 2, 3, 10, 11 and 138 — where the repeat codes 16 / 17 / 18 of the tree header
    change their token counts (deflate.c:141-189)."""
    lit = np.zeros(256, dtype=np.int64)
    lit[0:3] = 64          # 3 x length 3;   3, 4 zero
    lit[5:9] = 16          # 4 x length 5;   9 .. 11 zero
    lit[12:18] = 8         # 6 x length 6;   18 .. 27 zero
    lit[28:35] = 4         # 7 x length 7;   35 .. 45 zero
    lit[46:54] = 2         # 8 x length 8;   54 .. 191 zero (138)
    lit[192] = 128         # length 2
    lit[194] = 32          # length 4
    lit[196] = 2           # length 8
    lit[198] = 1           # length 9, as the end symbol
    assert lit.sum() == 511
    return lit


def families():
    """Every family of the issue but the plateaus' draws (plateau_family) — a list of Family."""
    rng = np.random.default_rng(1951)
    F = []
    # ---- Fibonacci counts: the 15-bit limit binds
    for n in (16, 17, 20, 30):
        F.append(Family("fibonacci", f"lit{n}", _at(256, zip(range(40, 40 + n), _fib(n)))))
    fl = _fib(29)
    F.append(Family("fibonacci", "length", _at(256, [(97, 10)]), fl, _spread(int(fl.sum()), 30)))
    fd = _fib(30)
    F.append(Family("fibonacci", "distance", _at(256, [(97, 10)]), _spread(int(fd.sum()), 29), fd))
    # ---- powers of two: a package ties a leaf at every level; all counts 1; all counts 7
    p2 = np.asarray([1] + [1 << k for k in range(18)], dtype=np.int64)
    F.append(Family("powers", "lit", _at(256, zip(range(10, 10 + len(p2)), p2))))
    pd = np.asarray([1] + [1 << k for k in range(16)], dtype=np.int64)
    F.append(Family("powers", "distance", _at(256, [(0, 3)]), _spread(int(pd.sum()), 29), _at(30, zip(range(len(pd)), pd))))
    F.append(Family("powers", "ones", np.ones(256, dtype=np.int64), _at(29, [(i, 2 if i == 0 else 1) for i in range(29)]),
                    np.ones(30, dtype=np.int64)))
    F.append(Family("powers", "sevens", np.full(256, 7, dtype=np.int64), np.full(29, 7, dtype=np.int64),
                    _at(30, [(i, 7) for i in range(29)])))
    # ---- every symbol in use: five items a lane, lists of 2n - 2 items
    ln, ds = rng.integers(1, 60, 29), rng.integers(1, 60, 30)
    _balance(rng, ln, ds)
    F.append(Family("all_used", "random", rng.integers(1, 60, 256), ln, ds))
    F.append(Family("all_used", "heavy_tail", rng.integers(1, 4, 256) * (1 + (np.arange(256) % 7 == 0) * 500),
                    _spread(3000, 29), _spread(3000, 30)))
    # ---- degenerate alphabets
    F.append(Family("degenerate", "one_literal", _at(256, [(65, 3000)])))
    F.append(Family("degenerate", "two_literals", _at(256, [(0, 2000), (255, 1500)])))
    F.append(Family("degenerate", "matches_only", None, _at(29, [(0, 900), (5, 700), (12, 800), (28, 100)]),
                    _at(30, [(0, 1000), (3, 500), (10, 900), (20, 100)])))
    F.append(Family("degenerate", "no_matches", _at(256, zip(range(32, 128), rng.integers(0, 120, 96)))))
    F.append(Family("degenerate", "one_distance_at_0", _at(256, [(120, 1500), (121, 40)]), _spread(1200, 29), _at(30, [(0, 1200)])))
    F.append(Family("degenerate", "one_distance_at_7", _at(256, [(120, 1500), (121, 40)]), _spread(1200, 29), _at(30, [(7, 1200)])))
    F.append(Family("degenerate", "one_distance_at_29", _at(256, [(1, 9)]), _at(29, [(3, 50)]), _at(30, [(29, 50)])))
    F.append(Family("degenerate", "two_distances", _at(256, [(7, 800)]), _spread(2500, 29), _at(30, [(3, 2000), (18, 500)])))
    F.append(Family("degenerate", "distance_29", _at(256, zip(range(60, 90), rng.integers(1, 90, 30))), _spread(600, 29),
                    _at(30, [(0, 300), (13, 260), (29, 40)])))
    F.append(Family("degenerate", "hlit_0", _at(256, [(0, 700), (200, 900), (255, 1100)])))
    F.append(Family("degenerate", "hlit_29", _at(256, zip(range(97, 123), rng.integers(1, 200, 26))), _at(29, [(0, 300), (28, 45)]),
                    _at(30, [(2, 200), (9, 145)])))
    # ---- every value: lengths 3 .. 258; distances at every base, base + 1 and the last of every symbol up to 32768
    dv = []
    for s, b in enumerate(DIST_BASE):
        last = (DIST_BASE[s + 1] if s < 29 else 32769) - 1
        dv += sorted({b, min(b + 1, last), last})
    lv = list(range(3, 259))
    n = max(len(lv), len(dv))
    F.append(Family("every_value", "lengths_distances", _at(256, [(10, 4), (13, 2)]),
                    matches=[(lv[i % len(lv)], dv[i % len(dv)]) for i in range(n)]))
    F.append(Family("every_value", "lengths_distances_x9", _at(256, [(10, 400)]),
                    matches=[(lv[(7 * i) % len(lv)], dv[i % len(dv)]) for i in range(9 * n)]))
    # ---- uniform literals: stored wins
    for k in (4, 16, 300):
        F.append(Family("uniform", f"x{k}", np.full(256, k, dtype=np.int64)))
    # ---- stores of exactly 1000 and 1001 symbols: either side of the fixed-tree switch (deflate.c:615)
    lit = _at(256, zip(range(97, 123), _spread(880, 26)))
    for n in (1000, 1001):
        F.append(Family("switch", f"n{n}", lit + _at(256, [(32, n - 980)]), _spread(100, 29), _spread(100, 30)))
    # (nearly flat: the dynamic tree's header costs more than it saves, whole store and pieces alike)
    for n in (1000, 1001):
        F.append(Family("switch", f"flat{n}", _at(256, zip(range(0, 144), _spread(n, 144)))))
    # ---- the split points of the repeat codes
    F.append(Family("repeat_splits", "complete_code", _repeat_splits()))
    F.append(Family("repeat_splits", "zero_run_149", _at(256, [(0, 5), (150, 9)]), _at(29, [(0, 3)]), _at(30, [(1, 3)])))
    return F


def all_families():
    return families() + [plateau_family(i) for i in range(PLATEAU_DRAWS)]


def near_limit(n, rare=3):
    """n symbols: one dominant literal and a rare second one (the sequences around the 2^22 limit)."""
    ll = np.full(n, 101, dtype=np.uint16)
    ll[np.linspace(0, n - 1, rare).astype(np.int64)] = 7
    return ll, np.zeros(n, dtype=np.uint16)


def ranges(m, seed, nrandom=10):
    """[(lstart, lend)] of a sequence of m symbols: the whole, single symbols, empty ranges (the reference prices them 0),
    ends on and beside the multiples of 1024 (the samples of the prefix counts), widths around 2048 (the direct-count
    threshold) and seeded random ranges, long and short."""
    rng = np.random.default_rng(seed)
    r = [(0, m), (0, 1), (m - 1, m), (m // 2, m // 2 + 1)]
    r += [(0, 0), (m // 2, m // 2), (1024, 1024), (m, m)]
    top = (m // 1024) * 1024
    for k in sorted({1024, 2048, 3072, top, (m // 2048) * 1024}):
        for e in (k - 1, k, k + 1):
            r += [(0, e), (e, m), (k // 2, e), (e, min(m, e + 1500))]
    for w in (2047, 2048, 2049):
        for a in (0, 1, 1023, 1024, m - w, m // 3):
            r.append((a, a + w))
    for _ in range(nrandom):
        r.append(tuple(sorted(rng.integers(0, m + 1, 2).tolist())))
        a = int(rng.integers(0, max(m, 1)))
        r.append((a, min(m, a + 1 + int(rng.integers(0, 700)))))
    out, seen = [], set()
    for a, b in r:
        if 0 <= a <= b <= m and (a, b) not in seen:
            seen.add((a, b))
            out.append((int(a), int(b)))
    return out
