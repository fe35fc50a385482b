"""Length arrays for the segmented trace (zmx_trace.h) and inputs for the segmented greedy walk (zmx_greedy.h), built
to stand ON the edges of both: the 4096-cell segments, their 258 possible entry cells and 516 entry states, the short
last segment the walk ends above or jumps over, the 2048-cell restage and the 64-cell windows of k_trace_emit, the
carry of a held match into the next segment, and the change points FollowPath resolves a length through.  With them
the plain references: TraceBackwards + FollowPath + histogram, and the lazy automaton of lz77.c:544-630, in Python over
the oracle's match records.  No device is involved; test_cpu_walk_cases.py asserts what the cases reach,
test_gpu_walk_edges.py holds the kernels to the references.

A length array cell h holds the length of the step that ENDS at cell h (squeeze.c:317); the walk starts at cell B.
The trace counts its segments from the top (segment s: cells (B - (s + 1) 4096, B - s 4096]), the greedy from the
bottom (segment s: positions [4096 s, 4096 (s + 1))).

Everything is computed once per process (functools.lru_cache) and must be left unchanged by its users."""
import functools

import numpy as np

import oracle_lib as ol
from zopfli_amd import generate

TS_SEG = 4096          # zmx_trace.h
TS_ENT = 258
TR_CHUNK = 2048        # zmx_kernels.h
EDGE_SIZES = ([1, 2, 3, 63, 64, 65, 257, 258, 259] + list(range(2039, 2050))
              + [4095, 4096, 4097, 4096 + 257, 4096 + 258, 4096 + 259, 8191, 8192, 8193])
CONST_STEPS = [1, 3, 4, 64, 129, 257, 258]
SHORT_R = [1, 2, 3, 257]
FILLINGS = ("zeros", "range", "path")

_LSYM = np.array([0, 0, 0] + [ol.length_symbol(l) for l in range(3, 259)])


@functools.lru_cache(maxsize=None)
def _dsym():
    return np.array([0] + [ol.dist_symbol(d) for d in range(1, 32769)])


def histogram(ll, dd):
    """288 litlen bins then 32 distance bins of a symbol run, no end symbol (lz77.c:98-149's counts)."""
    ll, dd = np.asarray(ll, dtype=np.int64), np.asarray(dd, dtype=np.int64)
    h = np.zeros(320, dtype=np.uint32)
    lit = dd == 0
    np.add.at(h, ll[lit], 1)
    np.add.at(h, _LSYM[ll[~lit]], 1)
    np.add.at(h, 288 + _dsym()[dd[~lit]], 1)
    return h


# ------------------------------------------------------------------------------------------------ match records
class Records:
    """The oracle's match records of block [instart, inend) of data."""

    def __init__(self, data, instart, inend):
        self.data, self.instart, self.inend = data, instart, inend
        t = ol.OracleTable(data, instart, inend)
        self.length, self.dist, self.off, self.cp_len, self.cp_dist = t.records()
        t.close()
        c = np.concatenate([[0], np.cumsum(self.cp_len >= 3)])
        self.ncp = c[self.off[1:]] - c[self.off[:-1]]          # change points of length 3 and more, per position

    def change_points(self, i):
        """(lengths, distances) of position i's change points of length 3 and more — what the device's record keeps
        (a byte holds length - 3): sublen[l] is the distance of the first one with length >= l."""
        a, b = int(self.off[i]), int(self.off[i + 1])
        keep = self.cp_len[a:b] >= 3
        return self.cp_len[a:b][keep], self.cp_dist[a:b][keep]

    def resolve(self, i, length):
        """(sublen[length] at position i or 0 if the record does not hold that length, index of the change point it
        resolves through, number of change points of the record)."""
        l, d = self.change_points(i)
        k = int(np.searchsorted(l, length))
        return (int(d[k]) if k < len(l) else 0), k, len(l)


@functools.lru_cache(maxsize=None)
def zeros_distance():
    """On zeros with zeros in front every length 3 .. 258 is valid at every position, at ONE distance: asked of the
    oracle once."""
    r = Records(bytes(1200), 300, 1200)
    assert np.all(r.length[:900 - 258] == 258)
    dist = set()
    for i in (0, 1, 299, 641):
        l, d = r.change_points(i)
        assert l.tolist() == [258]
        dist.add(int(d[0]))
    assert dist == {1}
    return 1


def _resolve_zeros(i, length):
    return zeros_distance(), 0, 1


# ------------------------------------------------------------------------------------------------ the trace reference
class ZeroOnPath(Exception):
    pass


class MissingLength(Exception):
    pass


def walk_back(la):
    """TraceBackwards (squeeze.c:317): the cells the walk visits, from cell B down."""
    heads, h = [], len(la) - 1
    while h > 0:
        heads.append(h)
        step = int(la[h])
        if step == 0:
            raise ZeroOnPath(h)
        assert step <= h and step != 2 and step <= 258, (h, step)
        h -= step
    return heads


def trace_reference(data, instart, la, resolve):
    """TraceBackwards + FollowPath (squeeze.c:338) + histogram of one block: a length below 3 is the literal at the
    step's start, otherwise the distance is sublen[length] there.  -> dict(ll, dd, hist, heads, via = [(change-point
    index, change points of the record)] per match symbol)."""
    heads = walk_back(la)
    ll, dd, via = [], [], []
    for h in reversed(heads):
        step = int(la[h])
        p = h - step
        if step < 3:
            ll.append(data[instart + p])
            dd.append(0)
        else:
            dist, k, ncp = resolve(p, step)
            if dist == 0:
                raise MissingLength((p, step))
            ll.append(step)
            dd.append(dist)
            via.append((k, ncp))
    ll, dd = np.array(ll, dtype=np.uint16), np.array(dd, dtype=np.uint16)
    return dict(ll=ll, dd=dd, hist=histogram(ll, dd), heads=heads, via=via)


def _restages(la, head, seg_lo):
    """How often k_trace_emit stages length_array cells for one segment: 64-cell windows from `head` down, a stage
    of up to TR_CHUNK cells whenever a window reaches below the staged ones."""
    lo = hi = n = 0
    while head > seg_lo:
        wb = max(head - 63, 0)
        if hi == 0 or wb < lo:
            lo = ((head - (TR_CHUNK - 8)) & ~7) if head > TR_CHUNK - 8 else 0
            hi = head
            n += 1
        lim = max(seg_lo + 1, wb)
        while head >= lim:
            head -= int(la[head])
    return n


def trace_segments(la, heads):
    """Per trace segment of the block: dict(s, cells, j = entry offset below the segment's top cell, skipped = the walk
    ended above it, nsym = symbols that end in it, restages)."""
    B = len(la) - 1
    asc = np.array(heads[::-1], dtype=np.int64)
    out = []
    for s in range((B + TS_SEG - 1) // TS_SEG):
        hi = B - s * TS_SEG
        lo = max(hi - TS_SEG, 0)
        k = int(np.searchsorted(asc, hi, side="right")) - 1
        entry = int(asc[k]) if k >= 0 else 0
        if entry <= lo:
            assert entry == 0 and lo == 0
            out.append(dict(s=s, cells=hi - lo, j=hi, skipped=True, nsym=0, restages=0))
            continue
        nsym = k + 1 - int(np.searchsorted(asc, lo, side="right"))
        out.append(dict(s=s, cells=hi - lo, j=hi - entry, skipped=False, nsym=nsym, restages=_restages(la, entry, lo)))
    return out


# ------------------------------------------------------------------------------------------------ path builders
def la_of_steps(steps):
    """The length array (zero off the path) of a forward sequence of steps."""
    la = np.zeros(int(sum(steps)) + 1, dtype=np.uint16)
    h = 0
    for step in steps:
        h += step
        la[h] = step
    return la


def const_path(B, L):
    """Constant steps L down from cell B; what is left at the bottom (B mod L cells) is literals."""
    return la_of_steps([1] * (B % L if L <= B else B) + [L] * (B // L))


def _fill(g, stride):
    """Steps that cover g cells: four literals at either end, strides in between."""
    top = min(4, g)
    g -= top
    bot = min(4, g)
    g -= bot
    mid = []
    while g >= stride + 3 or g == stride:
        mid.append(stride)
        g -= stride
    mid += [g] if g >= 3 else [1] * g
    return [1] * top + mid + [1] * bot


def edge_path(B, forced, stride):
    """A path that takes step L at cell a for every (a, L) of `forced`, with literals around each and strides between."""
    la = np.zeros(B + 1, dtype=np.uint16)
    h = B
    for a, L in sorted(forced, reverse=True) + [(0, 0)]:
        assert a <= h, (a, h)
        for step in _fill(h - a, stride):
            la[h] = step
            h -= step
        if L:
            assert 3 <= L <= min(h, 258)
            la[h] = L
            h -= L
    assert h == 0
    return la


def _crossing_length(j, v):
    """A step that lands j cells below a segment's top cell from above it is longer than j."""
    lo = max(3, j + 1)
    return lo + v % (259 - lo)


def entry_path(B, j):
    """One block of the entry-offset sweep: at every segment boundary one step crosses it and lands j cells below the
    top cell of the lower segment (j modulo its cells where it is shorter).  Where the bottom segment is short (fewer
    than 258 cells) and j is odd, the walk ends exactly at cell 0 from the segment above instead."""
    stride = (97, 64, 129, 33, 255)[j % 5]
    forced = []
    for s in range(1, (B + TS_SEG - 1) // TS_SEG):
        hi = B - s * TS_SEG
        cells = min(hi, TS_SEG)
        if cells < TS_ENT and j % 2 == 1:
            L = cells + 1 + (j // 2) % (258 - cells)
            forced.append((max(L, 3), max(L, 3)))
            continue
        jj = j % cells
        L = _crossing_length(jj, j * 37)
        forced.append((hi - jj + L, L))
    return edge_path(B, forced, stride)


def random_path(rec, B, seed):
    """A random valid path over real match records, walking forward: a literal, or (four times in five where there
    is a match) any length from 3 to the oracle's match length there — a change point drawn first, then a length that
    resolves through it, so that records of many change points are used through all of them.  Records of more than 8
    change points are rare (the pool of the device's records): where one lies within the next 258 positions the walk
    heads for it, by the step that lands on it or by literals, and takes a match there."""
    rng = np.random.default_rng(seed)
    la = np.zeros(B + 1, dtype=np.uint16)
    rich = np.flatnonzero(rec.ncp[:B] > 8)
    p = 0
    while p < B:
        step = 1
        k = int(np.searchsorted(rich, p + 1))
        if k < len(rich) and rich[k] - p <= 258:
            gap = int(rich[k]) - p
            step = gap if 3 <= gap <= rec.length[p] else 1
        elif rec.length[p] >= 3 and (rng.random() < 0.8 or rec.ncp[p] > 8):
            l, _ = rec.change_points(p)
            k = int(rng.integers(len(l)))
            step = int(rng.integers(max(3, int(l[k - 1]) + 1) if k else 3, int(l[k]) + 1))
        p += step
        la[p] = step
    return la


def fillings(la, other, seed):
    """The array with its off-path cells (zeros in `la`) as zeros, as other values from the valid range, and as the
    cells of `other`, a different valid path."""
    B = len(la) - 1
    on = la != 0
    r = np.random.default_rng(seed).integers(1, 259, B + 1)
    r = np.minimum(r, np.arange(B + 1))
    r[r == 2] = 1
    return dict(zeros=la, range=np.where(on, la, r).astype(np.uint16), path=np.where(on, la, other).astype(np.uint16))


# ------------------------------------------------------------------------------------------------ trace objects and cases
class TraceCase:
    """One call of the trace: a length array per block (zero off the path) and a second path per block."""

    def __init__(self, obj, name, las, others, seed):
        self.obj, self.name, self.las, self.others, self.seed = obj, name, las, others, seed

    def filled(self, which):
        return [fillings(la, other, self.seed + b)[which] for b, (la, other) in enumerate(zip(self.las, self.others))]

    @functools.lru_cache(maxsize=None)
    def reference(self):
        """Per block: trace_reference of the array (zero filling)."""
        o = self.obj
        return [trace_reference(o["data"], s, la, res) for (s, e), la, res in zip(o["blocks"], self.las, o["resolve"])]


def _zero_object(sizes):
    blocks, s = [], 300
    for n in sizes:
        blocks.append((s, s + n))
        s += n
    return dict(data=bytes(s), blocks=blocks, resolve=[_resolve_zeros] * len(blocks))


ZERO_SIZES = EDGE_SIZES[:12] + [0] + EDGE_SIZES[12:]           # an empty block between two others
ZERO_EDGES = [4096 + 259, 8192, 4096 + 1, 4096 + 2, 4096 + 3, 4096 + 257, 3 * 4096 + 1]
REAL = {"T": 30000, "M": 30000, "prefix8": 30000, "mut1k": 30000}
REAL_WINDOW = 12000
SEEDS = (1, 2, 3, 4)


def _real_data(name, n):
    if name in ("T", "M"):
        return generate(name, n)
    from test_gpu_match_adversarial import _make
    return _make(name, n).tobytes()


@functools.lru_cache(maxsize=None)
def trace_object(key):
    """dict(data, blocks, resolve = per block (position, length) -> (distance, change-point index, change points),
    cases = [TraceCase]) of one tables object: "zero_sizes" (constant steps over every edge block size), "zero_edges"
    (the entry-offset sweep with the short-segment endings) or one of REAL (random paths over real records, a window
    in front of the one block)."""
    if key == "zero_sizes":
        o = _zero_object(ZERO_SIZES)
        o["cases"] = [TraceCase(o, f"L{L}", [const_path(n, L) for n in ZERO_SIZES],
                                [const_path(n, 5 + (7 * L) % 200) for n in ZERO_SIZES], 1000 * L) for L in CONST_STEPS]
    elif key == "zero_edges":
        o = _zero_object(ZERO_EDGES)
        o["cases"] = [TraceCase(o, f"j{j}", [entry_path(n, j) for n in ZERO_EDGES],
                                [const_path(n, 3 + (11 * j) % 250) for n in ZERO_EDGES], 77 * j) for j in range(TS_ENT)]
    else:
        n = REAL[key]
        data = _real_data(key, n)
        rec = Records(data, REAL_WINDOW, n)
        o = dict(data=data, blocks=[(REAL_WINDOW, n)], resolve=[rec.resolve], records=rec)
        B = n - REAL_WINDOW
        o["cases"] = [TraceCase(o, f"{key}-seed{s}", [random_path(rec, B, s)], [random_path(rec, B, s + 100)], s) for s in SEEDS]
    return o


TRACE_OBJECTS = ("zero_sizes", "zero_edges") + tuple(REAL)


def missing_length_arrays(key):
    """Arrays over the real input `key` whose path takes, at one position, a length one above what the record there
    holds (a valid-range value: the host cannot know): [(what, la)] for a position without a match, one whose record has
    up to 8 change points and, where the input has one, one with more."""
    o = trace_object(key)
    rec = o["records"]
    B = len(rec.length)
    ncp = rec.ncp
    room = np.arange(B) + rec.length.astype(np.int64) + 1 <= B
    picks = {"none": (ncp == 0), "inline": (ncp >= 1) & (ncp <= 8) & (rec.length < 258),
             "pool": (ncp > 8) & (rec.length < 258)}
    out = []
    for what, mask in picks.items():
        at = np.flatnonzero(mask & room & (np.arange(B) > 5000))
        if len(at) == 0:
            continue
        p = int(at[0])
        step = max(int(rec.length[p]) + 1, 3)
        # a random path up to p, the step, a random path behind it
        la = np.zeros(B + 1, dtype=np.uint16)
        head = random_path_prefix(rec, p, 9)
        la[:p + 1] = head
        la[p + step] = step
        tail_rec = _Shifted(rec, p + step)
        la[p + step + 1:] = random_path(tail_rec, B - p - step, 10)[1:]
        out.append((what, p, step, la))
    return out


class _Shifted:
    """Records seen from block position `base` on."""

    def __init__(self, rec, base):
        self.rec, self.base = rec, base
        self.length = rec.length[base:]
        self.ncp = rec.ncp[base:]

    def change_points(self, i):
        return self.rec.change_points(self.base + i)


def random_path_prefix(rec, p, seed):
    """A random valid path over cells 0 .. p that ends exactly at cell p."""
    rng = np.random.default_rng(seed)
    la = np.zeros(p + 1, dtype=np.uint16)
    q = 0
    while q < p:
        step = 1
        if rec.length[q] >= 3 and rng.random() < 0.8:
            step = int(rng.integers(3, int(rec.length[q]) + 1))
            if q + step > p:
                step = 1
        q += step
        la[q] = step
    return la


# ------------------------------------------------------------------------------------------------ the greedy reference
def lazy_automaton(data, instart, length, dist):
    """ZopfliLZ77Greedy (lz77.c:544-630) over match records (length[i], dist[i] of block position i): (litlens, dists,
    visited = [(position, held)] in order, held = {position: "match" | "literal"}: what a visit with a held match
    emitted for position - 1)."""
    B = len(length)
    ll, dd, visited, held_out = [], [], [], {}
    i, held, prev_len, prev_dist = 0, False, 0, 0

    def score(l, d):
        return l - 1 if d > 1024 else l                                   # lz77.c:265-271

    while i < B:
        visited.append((i, held))
        leng, d = int(length[i]), int(dist[i])
        sc = score(leng, d)
        if held:                                                           # lz77.c:581-607
            held = False
            if sc > score(prev_len, prev_dist) + 1:
                ll.append(data[instart + i - 1])
                dd.append(0)
                held_out[i] = "literal"
                if sc >= 3 and leng < 258:
                    held, prev_len, prev_dist = True, leng, d
                    i += 1
                    continue
            else:
                ll.append(prev_len)
                dd.append(prev_dist)
                held_out[i] = "match"
                i += prev_len - 1
                continue
        elif sc >= 3 and leng < 258:                                       # lz77.c:608-613
            held, prev_len, prev_dist = True, leng, d
            i += 1
            continue
        if sc >= 3:                                                        # lz77.c:618-629
            ll.append(leng)
            dd.append(d)
            i += leng
        else:
            ll.append(data[instart + i])
            dd.append(0)
            i += 1
    return np.array(ll, dtype=np.uint16), np.array(dd, dtype=np.uint16), visited, held_out


def greedy_entries(B, visited):
    """Per greedy segment s >= 1 of a block: (j, held) = the state the walk enters it in, or ("jumped", its positions)
    when no position of it is visited."""
    pos = np.array([v[0] for v in visited], dtype=np.int64)
    out = []
    for s in range(1, (B + TS_SEG - 1) // TS_SEG):
        lo, hi = s * TS_SEG, min((s + 1) * TS_SEG, B)
        k = int(np.searchsorted(pos, lo))
        if k == len(pos) or pos[k] >= hi:
            out.append(("jumped", hi - lo))
        else:
            out.append((int(pos[k]) - lo, bool(visited[k][1])))
    return out


# ------------------------------------------------------------------------------------------------ planted greedy inputs
PLANTED = ([("end", j) for j in range(TS_ENT)] + [("held_match", 0), ("held_literal", 0)]
           + [("jump", r) for r in SHORT_R])
PLANTED_GROUP = 22
PLANTED_GROUPS = (len(PLANTED) + PLANTED_GROUP - 1) // PLANTED_GROUP
PLANTED_SIZE = TS_SEG + 300


def _plant_copy(a, p, L, src):
    """a[p : p + L] becomes a copy of a[src : src + L] that can be extended neither way."""
    a[p:p + L] = a[src:src + L]
    a[p - 1] = a[src - 1] ^ 0x55
    if p + L < len(a):
        a[p + L] = a[src + L] ^ 0x55


def _planted_block(kind, arg, seed):
    """One block of random bytes with the planted copies of one case; the source lies a few hundred positions back
    in the same random bytes, so it is the only one.  -> (bytes, what greedy_entries must show)."""
    rng = np.random.default_rng(seed)
    lo = TS_SEG
    if kind == "jump":                      # a top segment of `arg` positions, jumped over by a match that ends at the block end
        size = lo + arg
        a = rng.integers(0, 256, size, dtype=np.uint8)
        L = max(arg + 1, 3) + (seed % 7 if arg < 200 else 0)
        _plant_copy(a, size - L, L, size - L - 400)
        return a, ("jumped", arg)
    a = rng.integers(0, 256, PLANTED_SIZE, dtype=np.uint8)
    if kind == "end":                       # a match that starts before lo and ends at lo + arg
        L = _crossing_length(arg, seed)
        _plant_copy(a, lo + arg - L, L, lo + arg - L - 400)
        return a, (arg, False)
    if kind == "held_match":                # held at lo - 1, and emitted at lo: the match one shorter there does not beat it
        _plant_copy(a, lo - 1, 20, lo - 401)
        return a, (0, True)
    # held_literal: a match of 5 held at lo - 1 is replaced by one of 20 that starts at lo; lo - 1 becomes a literal
    s1, s2 = lo - 600, lo - 300
    a[s1 + 1:s1 + 5] = a[s2:s2 + 4]
    a[s1 + 5] = a[s2 + 4] ^ 0x55
    a[s2 - 1] = a[s1] ^ 0x33
    a[lo - 1] = a[s1]
    a[lo - 2] = a[s1 - 1] ^ 0x55
    a[lo:lo + 20] = a[s2:s2 + 20]
    a[lo + 20] = a[s2 + 20] ^ 0x55
    return a, (0, True)


@functools.lru_cache(maxsize=None)
def planted_group(g):
    """dict(data, blocks, specs, refs = per block dict(ll, dd, hist, visited, held, entries)) of PLANTED[22 g : 22 g + 22],
    one block each, back to back.  Random bytes match each other by chance now and then (three equal bytes some
    thousand positions apart); a block whose planted state such a match disturbs is drawn again with the next seed."""
    specs = PLANTED[g * PLANTED_GROUP:(g + 1) * PLANTED_GROUP]
    data, blocks, refs = b"", [], []
    for n, (kind, arg) in enumerate(specs):
        for attempt in range(20):
            a, want = _planted_block(kind, arg, 100000 * g + 100 * n + attempt)
            cand = data + a.tobytes()
            s, e = len(data), len(cand)
            rec = Records(cand, s, e)
            ll, dd, visited, held = lazy_automaton(cand, s, rec.length, rec.dist)
            entries = greedy_entries(e - s, visited)
            ok = entries == [want]
            if kind.startswith("held"):
                ok = ok and held.get(TS_SEG) == kind[5:]
            if ok:
                break
        else:
            raise AssertionError(f"planted case {kind} {arg} is not reached")
        data = cand
        blocks.append((s, e))
        refs.append(dict(ll=ll, dd=dd, hist=histogram(ll, dd), visited=visited, held=held, entries=entries))
    return dict(data=data, blocks=blocks, specs=specs, refs=refs)


CLASS_BLOCKS = ("T", "M")


@functools.lru_cache(maxsize=None)
def class_blocks(cls):
    """dict(data, blocks): class data cut into blocks of the edge sizes, 300 bytes in front of the first."""
    blocks, s = [], 300
    for n in EDGE_SIZES:
        blocks.append((s, s + n))
        s += n
    return dict(data=generate(cls, s), blocks=blocks)
