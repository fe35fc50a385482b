"""Inputs and cost models that STEER the squeeze, for test_cpu_steer_cases.py (what they reach, asserted with the CPU
oracle and plain Python alone) and the GPU files test_gpu_mincost_edges.py, test_gpu_bit_writer_limits.py and
test_gpu_verify_reports.py.

There is no entry point that uploads an LZ77 store: a store of a chosen shape is what zmx_squeeze_run leaves behind
for a chosen cost model over a built input.  Two recipes (every cost within [0, 24] bits, the range
CalculateStatistics, squeeze.c:392, can produce itself):

  all literals   literal costs 2^-5, every length and distance symbol 16: the optimal parse is all literals whatever
                 the data, so nsym == inend - instart exactly (2047, 2048, 2049, 4096 and 64 * 2048 + 1 symbols)
  48-bit tile    20000 random bytes repeated with period 20000; every symbol costs 12, length symbols 281..284 cost 1,
                 symbol 285 costs 24, distance symbol 29 costs 1: every match has length 131..257 (5 extra bits) at
                 distance 20000 (13 extra bits), so with 15-bit codes every symbol takes 15 + 5 + 15 + 13 = 48 bits,
                 the most a deflate symbol can take; 2068 of them fill a 2048-symbol tile of the device's bit writer
                 (zmx_encode.h) to the last bit of its buffer.  The `mixed` variant breaks the period at irregular
                 places: the literals in between move the symbol starts over every bit residue.

The sub-mincost cases pass GetBestLengths (squeeze.c:217) a mincost ABOVE GetCostModelMinCost of the model (the
oracle defines what that means: the test costs[j + k] <= mincost + costs[j] of squeeze.c:293 with the value given),
or a model in which a match weight lies below GetCostModelMinCost itself through rounding.

References are computed once per process (functools.lru_cache) and must be left unchanged by their users."""
import functools

import numpy as np

import oracle_lib as ol
from zopfli_amd import generate

ENC_TILE = 2048                       # symbols per tile of the device's bit writer (zmx_encode.h ENC_TILE)
LEN_EXTRA = np.array([0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0])      # by length symbol - 257
DIST_EXTRA = np.array([0] * 4 + [s // 2 - 1 for s in range(4, 30)])                        # by distance symbol


# ------------------------------------------------------------------------------------------------ cost models
def all_literal_model():
    """(ll[288], d[32]): literals 2^-5, everything else 16."""
    ll = np.full(288, 16.0)
    ll[:256] = 2.0 ** -5
    return ll, np.full(32, 16.0)


def tile48_model():
    ll = np.full(288, 12.0)
    ll[281:285] = 1.0
    ll[285] = 24.0
    d = np.full(32, 12.0)
    d[29] = 1.0
    return ll, d


def rounding_model(hist320):
    """Entropy costs of a histogram with four symbols overwritten so that a match weight lies below
    GetCostModelMinCost (squeeze.c:163) itself: at length 3 the distance symbols 0 and 1 tie (16 + (1 - 2^-52) rounds
    to 17), the first wins, so mincost = cost(length 4, distance 1) = 1.25 — and the weight of (length 4, distance 2)
    is 0.25 + (1 - 2^-52) = 1.25 - 2^-52."""
    ll, d = ol.entropy_costs(hist320)
    ll, d = ll.copy(), d.copy()
    ll[257], ll[258], d[0], d[1] = 16.0, 0.25, 1.0, 1.0 - 2.0 ** -52
    return ll, d


def weights_below(ll, d, mincost):
    """[(length symbol, distance symbol)] of the match weights below `mincost`, in GetCostStat's arithmetic
    (squeeze.c:146-157: (lbits + dbits) as int, + ll, + d)."""
    out = []
    for ls in range(257, 286):
        for ds in range(30):
            w = (float(int(LEN_EXTRA[ls - 257]) + int(DIST_EXTRA[ds])) + ll[ls]) + d[ds]
            if w < mincost:
                out.append((ls, ds))
    return out


def cost_rows(models):
    """[(ll, d)] per block -> cost[nb, 320], mincost[nb] = GetCostModelMinCost."""
    cost = np.zeros((len(models), 320))
    mincost = np.zeros(len(models))
    for b, (ll, d) in enumerate(models):
        cost[b, :288], cost[b, 288:] = ll, d
        mincost[b] = ol.model_min_cost(ll, d)
    return cost, mincost


# ------------------------------------------------------------------------------------------------ inputs
def all_literal_input():
    """(data, blocks): blocks of 2047, 2048, 2049 and 4096 bytes over a 4-letter alphabet, then 64 * 2048 + 1 random
    bytes: with all_literal_model() each is a store of exactly that many literals."""
    rng = np.random.default_rng(4)
    small = rng.choice(np.frombuffer(b"acgt", dtype=np.uint8), 2047 + 2048 + 2049 + 4096)
    data = small.tobytes() + rng.integers(0, 256, 64 * ENC_TILE + 1, dtype=np.uint8).tobytes()
    blocks, s = [], 0
    for n in (2047, 2048, 2049, 4096, 64 * ENC_TILE + 1):
        blocks.append((s, s + n))
        s += n
    assert s == len(data)
    return data, blocks


def tile48_input(mixed=False):
    """(data, blocks): 20000 random bytes, then 2048 * 257 + 5000 bytes that repeat them with period 20000; the block
    is everything behind the first period.  mixed: a byte that differs from the one 20000 before it every 132 .. 900
    bytes (now and then two in a row): matches end there and a literal stands between them."""
    rng = np.random.default_rng(48)
    period, more = 20000, ENC_TILE * 257 + 5000
    a = np.zeros(period + more, dtype=np.uint8)
    a[:period] = rng.integers(0, 256, period, dtype=np.uint8)
    breaks = np.zeros(period + more, dtype=bool)
    if mixed:
        p = period + 300
        while p + 2 < len(a):
            breaks[p] = True
            if rng.integers(0, 5) == 0:
                breaks[p + 1] = True
            p += int(rng.integers(132, 901))
    for s in range(period, period + more, period):
        e = min(s + period, period + more)
        a[s:e] = a[s - period:e - period]
        a[s:e][breaks[s:e]] ^= 0x55
    return a.tobytes(), [(period, period + more)]


# ------------------------------------------------------------------------------------------------ the oracle, cached
@functools.lru_cache(maxsize=None)
def _tables(key):
    data, blocks = key
    return [ol.OracleTable(data, s, e) for (s, e) in blocks]


def oracle_tables(data, blocks):
    return _tables((data, tuple(blocks)))


def oracle_run(data, blocks, cost, mincost):
    """[(length_array, litlens, dists)] per block: GetBestLengths + TraceBackwards + FollowPath of the oracle."""
    tabs = oracle_tables(data, blocks)
    return [tabs[b].squeeze_run(cost[b, :288], cost[b, 288:], mincost[b]) for b in range(len(blocks))]


def greedy_hists(data, blocks):
    return [ol.histogram(*t.greedy()) for t in oracle_tables(data, blocks)]


@functools.lru_cache(maxsize=None)
def steered(name):
    """The steered stores: dict(data, blocks, cost, mincost, runs = oracle_run(...)) for "literals", "tile48" and
    "tile48_mixed"."""
    if name == "literals":
        data, blocks = all_literal_input()
        model = all_literal_model()
    else:
        data, blocks = tile48_input(mixed=name == "tile48_mixed")
        model = tile48_model()
    cost, mincost = cost_rows([model] * len(blocks))
    return dict(data=data, blocks=blocks, cost=cost, mincost=mincost, runs=oracle_run(data, blocks, cost, mincost))


# (name, class, size, blocks, delta): entropy costs of the greedy histogram, mincost = GetCostModelMinCost + delta.
# Block shapes as test_gpu_parity.TABLE_CASES: a window before instart, runs across a block end, tiny and empty blocks.
INFLATED = [
    ("T-d1", "T", 60000, [(0, 60000)], 1.0),
    ("T-d3", "T", 60000, [(0, 60000)], 3.0),
    ("B-d0.25", "B", 60000, [(0, 60000)], 0.25),
    ("P-d3", "P", 66000, [(33000, 66000)], 3.0),
    ("Z-d10", "Z", 90000, [(0, 45001), (45001, 90000)], 10.0),      # no difference at delta <= 6 on this class
    ("M-d3", "M", 150000, [(0, 3), (3, 5), (5, 5), (5, 100000), (100000, 150000)], 3.0),
]
# (name, class, size, blocks): rounding_model of the greedy histogram, mincost = GetCostModelMinCost exactly
ROUNDING = [
    ("T", "T", 60000, [(0, 60000)]),
    ("B", "B", 60000, [(10000, 60000)]),
    ("Z", "Z", 90000, [(0, 45001), (45001, 90000)]),
]
# the runs of one table set, in this order and in alternating slots: per block the delta added to mincost
STATE_CASE = ("T", 90000, [(0, 30000), (30000, 60000), (60000, 90000)])
STATE_RUNS = [(0.0, 0.0, 0.0), (3.0, 3.0, 3.0), (0.0, 0.0, 0.0), (0.0, 3.0, 0.0), (0.0, 0.0, 0.0)]


@functools.lru_cache(maxsize=None)
def inflated(name):
    """dict(data, blocks, cost, mincost_true, mincost, runs_true, runs) of an INFLATED case."""
    _, cls, n, blocks, delta = next(c for c in INFLATED if c[0] == name)
    data = generate(cls, n)
    cost, true = cost_rows([ol.entropy_costs(h) for h in greedy_hists(data, blocks)])
    return dict(data=data, blocks=blocks, cost=cost, mincost_true=true, mincost=true + delta,
                runs_true=oracle_run(data, blocks, cost, true), runs=oracle_run(data, blocks, cost, true + delta))


@functools.lru_cache(maxsize=None)
def rounding(name):
    """dict(data, blocks, cost, mincost, runs, runs_zero) of a ROUNDING case (runs_zero: the oracle with mincost 0)."""
    _, cls, n, blocks = next(c for c in ROUNDING if c[0] == name)
    data = generate(cls, n)
    cost, mincost = cost_rows([rounding_model(h) for h in greedy_hists(data, blocks)])
    return dict(data=data, blocks=blocks, cost=cost, mincost=mincost, runs=oracle_run(data, blocks, cost, mincost),
                runs_zero=oracle_run(data, blocks, cost, np.zeros(len(blocks))))


@functools.lru_cache(maxsize=None)
def state_runs():
    """dict(data, blocks, cost, mincost_true, runs = [(mincost, oracle_run)] per STATE_RUNS entry)."""
    cls, n, blocks = STATE_CASE
    data = generate(cls, n)
    cost, true = cost_rows([ol.entropy_costs(h) for h in greedy_hists(data, blocks)])
    runs = [(true + np.array(dl), oracle_run(data, blocks, cost, true + np.array(dl))) for dl in STATE_RUNS]
    return dict(data=data, blocks=blocks, cost=cost, mincost_true=true, runs=runs)


def differing_positions(runs_a, runs_b):
    """Positions at which the length arrays of two oracle_run results differ, per block."""
    return [int(np.count_nonzero(a[0][1:] != b[0][1:])) for a, b in zip(runs_a, runs_b)]


def assert_run_equals_oracle(t, blocks, slot, nsym, hist, runs, tag):
    """A zmx_squeeze_run on Tables `t` against oracle_run's result: length array, store and histogram."""
    for b, (s, e) in enumerate(blocks):
        la, oll, odd = runs[b]
        if e > s:
            gla = t.length_array(b)
            bad = np.nonzero(gla[1:] != la[1:])[0]
            assert len(bad) == 0, f"{tag} block {b}: length_array differs at {len(bad)} positions, first {1 + int(bad[0])}"
        assert nsym[b] == len(oll), f"{tag} block {b}: nsym {nsym[b]} against {len(oll)}"
        gll, gdd = t.store(b, slot, nsym[b])
        assert np.array_equal(gll, oll) and np.array_equal(gdd, odd), f"{tag} block {b}: store"
        assert np.array_equal(hist[b], ol.histogram(oll, odd)), f"{tag} block {b}: histogram"


# ------------------------------------------------------------------------------------------------ code tables
def codes_15bit(seed):
    """uint32[320]: a random 15-bit pattern | 15 << 16 on every symbol (zmx_encode_blocks does not ask for a prefix code)."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 1 << 15, 320).astype(np.uint32) | np.uint32(15 << 16)).astype(np.uint32)


def codes_mixed(seed):
    """Lengths 1 .. 15, each of them on some symbol, random patterns of that many bits."""
    rng = np.random.default_rng(seed)
    n = rng.integers(1, 16, 320)
    n[rng.permutation(320)[:15]] = np.arange(1, 16)
    return ((rng.integers(0, 1 << 15, 320) & ((1 << n) - 1)) | (n << 16)).astype(np.uint32)


def codes_sparse(litlens, dists, seed):
    """codes_mixed on the symbols the store uses (and the end symbol), length 0 and no bits on all others."""
    used = np.zeros(320, dtype=bool)
    ls, ds = symbols_of(litlens, dists)
    used[ls] = True
    used[288 + ds[ds >= 0]] = True
    used[256] = True
    return np.where(used, codes_mixed(seed), 0).astype(np.uint32)


# ------------------------------------------------------------------------------------------------ bookkeeping
def symbols_of(litlens, dists):
    """Per symbol of a store: the litlen symbol, and the distance symbol or -1 for a literal."""
    litlens, dists = np.asarray(litlens, dtype=np.int64), np.asarray(dists, dtype=np.int64)
    m = dists != 0
    ls = np.where(m, 256 + np.searchsorted(np.asarray(ol._LEN_BASE), np.where(m, litlens, 3), side="right"), litlens)
    first = np.array([1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
                      4097, 6145, 8193, 12289, 16385, 24577])
    ds = np.where(m, np.searchsorted(first, np.where(m, dists, 1), side="right") - 1, -1)
    return ls, ds


def symbol_bits(litlens, dists, codes):
    """Bits every symbol of a store takes under `codes` (code lengths + extra bits), as AddLZ77Data writes them."""
    ls, ds = symbols_of(litlens, dists)
    n = np.asarray(codes, dtype=np.int64) >> 16
    m = ds >= 0
    bits = n[ls]
    bits = bits + np.where(m, LEN_EXTRA[np.where(m, ls - 257, 0)] + n[288 + np.where(m, ds, 0)] + DIST_EXTRA[np.where(m, ds, 0)], 0)
    return bits


def tile_starts(bits):
    """Where each symbol starts in ITS TILE's bit buffer (the device ORs a tile's symbols into a buffer of its own from
    bit 0), and per tile the bits of its symbols (= where the end symbol goes in the last tile)."""
    bits = np.asarray(bits, dtype=np.int64)
    ntiles = len(bits) // ENC_TILE + 1
    start = np.zeros(len(bits), dtype=np.int64)
    total = np.zeros(ntiles, dtype=np.int64)
    for t in range(ntiles):
        b = bits[t * ENC_TILE:(t + 1) * ENC_TILE]
        start[t * ENC_TILE:t * ENC_TILE + len(b)] = np.cumsum(b) - b
        total[t] = b.sum()
    return start, total


def three_word_shifts(bits):
    """The shifts sh = start & 31 of the symbols that reach a third 32-bit word of their tile's buffer (sh + n > 64)."""
    start, _ = tile_starts(bits)
    sh = start & 31
    return set(int(x) for x in np.unique(sh[sh + np.asarray(bits) > 64]))


def longest_run_of(bits, value):
    """Length of the longest run of consecutive symbols of exactly `value` bits."""
    best = cur = 0
    for x in (np.asarray(bits) == value).tolist():
        cur = cur + 1 if x else 0
        best = max(best, cur)
    return best


def write_symbols(py_symbol_bits, litlens, dists, codes, bit_start):
    """The bit-by-bit Python writer of test_gpu_parity (`py_symbol_bits`: AddLZ77Data + end symbol over one big integer)
    applied tile by tile, so that a store of 130 000 symbols does not shift a 2 Mbit integer 130 000 times: every piece
    but the last is written with an end symbol of no bits, at the bit where the piece before it stopped.
    Returns (bytes, nbits) like the writer itself."""
    codes = np.asarray(codes, dtype=np.uint32)
    inner = codes.copy()
    inner[256] = 0
    n = len(litlens)
    out = bytearray()
    pos = bit_start
    for t in range(n // ENC_TILE + 1):
        last = t == n // ENC_TILE
        piece, nb = py_symbol_bits(litlens[t * ENC_TILE:(t + 1) * ENC_TILE], dists[t * ENC_TILE:(t + 1) * ENC_TILE],
                                   codes if last else inner, pos & 7)
        at = pos >> 3
        if len(out) < at + len(piece):
            out.extend(bytes(at + len(piece) - len(out)))
        for i, x in enumerate(piece):
            out[at + i] |= x
        pos += nb
    return bytes(out), pos - bit_start


def end_symbol_prefixes(bits):
    """{sh: n} for sh = 18 .. 31: the longest prefix of n symbols after which the end symbol starts at shift sh of its
    tile's buffer, so that its 15 bits cross into the next word."""
    start, _ = tile_starts(bits)
    out = {}
    for n in range(len(start)):
        sh = int(start[n]) & 31
        if sh >= 18:
            out[sh] = n
    return out


# ------------------------------------------------------------------------------------------------ ZopfliVerifyLenDist
def verify_len_dist(data, instart, inend, litlens, dists):
    """ZopfliVerifyLenDist (lz77.c:270-295) over a whole store of block [instart, inend): None, or (index, reason) of the
    FIRST symbol that fails — 1: length or distance out of range, 2: the bytes are not the input's — or (nsym, 3) when
    every symbol holds and they do not add up to the block."""
    pos = instart
    for i, (l, d) in enumerate(zip(np.asarray(litlens).tolist(), np.asarray(dists).tolist())):
        if d == 0:
            if l > 255:
                return i, 1
            if pos >= inend or data[pos] != l:
                return i, 2
            pos += 1
        else:
            if l < 3 or l > 258 or d > 32768 or d > pos or pos + l > inend:
                return i, 1
            if data[pos:pos + l] != bytes(data[pos - d + k] for k in range(l)) and any(
                    data[pos + k] != data[pos + k - d] for k in range(l)):
                return i, 2
            pos += l
    return None if pos == inend else (len(litlens), 3)
