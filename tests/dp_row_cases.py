"""The DP row layout that the table build writes once for every squeeze run — dph[] (k_rowscan), codes[] (k_codes), the
window records wmeta[] / winflag[] / winroff[] (k_mkdesc); Tables.dp_rows reads them back — as a plain reference in
numpy, and inputs built to stand ON the edges of those kernels: block sizes around their steps and tiles, rows cut by
the block end, records of 0 .. 252 change points on either side of the inline / pool boundary, sub-chunks of k_codes
that fill EG_CAP to the slot, every literal, length and distance-symbol boundary, the four inequalities of the
long-run shortcut flag, run rows around the codeless threshold, every window kind.

reference_layout is written from squeeze.c, lz77.c and the comments of include/zopfli_amd.h over the oracle's match
records (OracleTable.records), zo_same and the bytes; best_lengths walks its rows as GetBestLengths (squeeze.c:217)
does, so that test_cpu_dp_row_cases.py can hold the reference itself to the oracle's zo_get_best_lengths.  No device
is involved here; test_cpu_dp_row_cases.py asserts what every builder reaches, test_gpu_dp_rows.py holds the kernels
to the reference.

Everything is computed once per process (functools.lru_cache) and must be left unchanged by its users."""
import functools

import numpy as np

import oracle_lib as ol
from zopfli_amd import generate

MAX_MATCH = 258
EG_CAP = 2048            # zmx_kernels.h: edges a wave of k_codes expands at a time
WM = 40                  # zmx_dp_build.h: words per window record
WF_CODELESS = 0x100
CODELESS_FROM = 64       # a run row of this many edges or more takes no codes
INLINE_CPS = 8           # change points a device record holds itself; more go to the pool
NO_CODE = 0xffff         # never a code: codes are multiples of 8

_LSYM = np.array([0, 0, 0] + [ol.length_symbol(l) for l in range(3, MAX_MATCH + 1)], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _dsym():
    return np.array([0] + [ol.dist_symbol(d) for d in range(1, 32769)], dtype=np.int64)


def dist_boundaries():
    """The first and the last distance of each of the 30 distance symbols that a match can have: lz77.c:464 walks the
    chain while dist < 32768, so the last one is 32767."""
    d = _dsym()
    out = []
    for s in range(30):
        at = np.flatnonzero(d[1:] == s) + 1
        out += [int(at[0]), min(int(at[-1]), 32767)]
    return sorted(set(out))


# ------------------------------------------------------------------------------------------------ the reference
def reference_layout(data, instart, inend, codeless):
    """What Tables.dp_rows(block) must return for block [instart, inend) of data, as a dict of the same names, and with
    it: "wmeta_defined" (bool [W, 40]) and "win_defined" (bool [W]), the words anybody may assert on; "lay" (slots per
    row); "edge_len" / "edge_dist" (per slot of codes[]: the match an edge stands for, 0 for literals and dead slots);
    "length", "dist", "ncp" (change points of length 3 and more) and "same" per position."""
    B = inend - instart
    W = (B + 31) // 32 + 1
    wmeta = np.zeros((W, WM), dtype=np.uint32)
    if B == 0:
        z = np.zeros(0, dtype=np.uint32)
        return dict(roff=z, flags=z, kend=z, shortcut=z, run_row=z, literal=z, codeless=z, block_edges=0,
                    codes=np.zeros(0, dtype=np.uint16), winflag=np.zeros(W, dtype=np.uint32),
                    winroff=np.zeros(W, dtype=np.uint32), wmeta=wmeta, wmeta_defined=np.zeros((W, WM), dtype=bool),
                    win_defined=np.zeros(W, dtype=bool), lay=z, edge_len=np.zeros(0, dtype=np.uint16),
                    edge_dist=np.zeros(0, dtype=np.uint16), length=z, dist=z, ncp=z, same=z)
    t = ol.OracleTable(data, instart, inend)
    length, dist, off, cp_len, cp_dist = t.records()
    same = np.array([t.lib.zo_same(t.h, p) for p in range(instart, inend)], dtype=np.int64)
    t.close()
    length, dist = length.astype(np.int64), dist.astype(np.int64)
    byte = np.frombuffer(data, dtype=np.uint8)[instart:inend].astype(np.int64)
    j = np.arange(B, dtype=np.int64)

    # the change points of length 3 and more, each with its position
    keep = cp_len >= 3
    kp = np.repeat(j, np.diff(off))[keep]
    kl, kd = cp_len[keep].astype(np.int64), cp_dist[keep].astype(np.int64)
    ncp = np.bincount(kp, minlength=B)

    kend = np.minimum(length, B - j)                                    # squeeze.c:286
    kend[kend < 3] = 1
    run_row = (length >= 3) & (dist == 1) & (ncp == 1)
    back = same[np.maximum(j - MAX_MATCH, 0)]
    shortcut = (same > 2 * MAX_MATCH) & (j > MAX_MATCH + 1) & (j + 2 * MAX_MATCH + 1 < B) & (back > MAX_MATCH)   # squeeze.c:251-258
    nocodes = run_row & (kend >= CODELESS_FROM) & bool(codeless)
    lay = np.where(nocodes, 0, kend)
    roff = np.cumsum(lay) - lay
    edges = int(lay.sum())
    flags = kend | shortcut.astype(np.int64) << 16 | run_row.astype(np.int64) << 17 | byte << 18 | nocodes.astype(np.int64) << 26

    # the codes: every slot of every row is written exactly once
    codes = np.full(edges, NO_CODE, dtype=np.int64)
    edge_len = np.zeros(edges, dtype=np.uint16)
    edge_dist = np.zeros(edges, dtype=np.uint16)
    rows = ~nocodes
    codes[roff[rows]] = (1 + byte[rows]) * 8                            # squeeze.c:278
    codes[roff[rows & (kend >= 3)] + 1] = 0                             # no edge of length 2
    if len(kp):
        first = np.concatenate([[True], kp[1:] != kp[:-1]])
        lo = np.where(first, 2, np.concatenate([[0], kl[:-1]])) + 1     # a change point serves the lengths above the one before it
        lo = np.maximum(lo, 3)
        hi = np.minimum(kl, kend[kp])
        cnt = np.where(rows[kp], np.maximum(hi - lo + 1, 0), 0)
        ramp = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        k = np.repeat(lo, cnt) + ramp
        d = np.repeat(kd, cnt)
        at = np.repeat(roff[kp], cnt) + k - 1
        assert np.all(codes[at] == NO_CODE)
        codes[at] = (257 + 30 * (_LSYM[k] - 257) + _dsym()[d]) * 8
        edge_len[at] = k
        edge_dist[at] = d
    assert not np.any(codes == NO_CODE), "a slot of the reference layout has no code"

    # the 32-position windows
    nw = W - 1
    P = nw * 32

    def padded(x, fill=0):
        return np.concatenate([np.asarray(x, dtype=np.int64), np.full(P - B, fill, dtype=np.int64)]).reshape(nw, 32)

    inside = padded(np.ones(B), 0).astype(bool)
    u = np.arange(32, dtype=np.int64)[None, :]
    K, R = padded(kend), padded(roff)
    reach = K + u
    flagged = padded(shortcut).astype(bool)
    wide_run = padded(run_row & (kend >= CODELESS_FROM)).astype(bool)
    kind1 = inside.all(1) & ~flagged.any(1) & (reach < 64).all(1)
    kind0 = ~inside.all(1) | flagged.any(1) | wide_run.any(1)
    kind = np.where(kind1, 1, np.where(kind0, 0, np.where((reach < 128).all(1), 2, 3)))
    kind = kind | np.where(padded(nocodes).astype(bool).any(1), WF_CODELESS, 0)
    first_roff = R[:, 0]
    words = ((R - first_roff[:, None] + 32 - (u + 1)) << 16) | K
    wmeta[:nw, :32] = np.where(inside, words, 0)
    wmeta[:nw, 32] = first_roff
    wmeta[:nw, 33] = np.concatenate([first_roff[1:], [edges]])
    wmeta[:nw, 34] = kind
    wmeta[nw, 32] = wmeta[nw, 33] = edges
    wmeta[nw, 34] = 0
    defined = np.zeros((W, WM), dtype=bool)
    defined[:nw, :35] = True
    defined[nw, 32:35] = True
    u32 = lambda x: np.asarray(x).astype(np.uint32)    # noqa: E731
    return dict(roff=u32(roff), flags=u32(flags), kend=u32(kend), shortcut=u32(shortcut), run_row=u32(run_row),
                literal=u32(byte), codeless=u32(nocodes), block_edges=edges, codes=codes.astype(np.uint16),
                winflag=wmeta[:, 34].copy(), winroff=wmeta[:, 32].copy(), wmeta=wmeta, wmeta_defined=defined,
                win_defined=np.ones(W, dtype=bool), lay=u32(lay), edge_len=edge_len, edge_dist=edge_dist,
                length=u32(length), dist=u32(dist), ncp=u32(ncp), same=u32(same))


def first_difference(got, want):
    """None, or what differs first between Tables.dp_rows(b) and reference_layout(...): the array, the position, slot
    or window word, and both values."""
    if int(got["block_edges"]) != int(want["block_edges"]):
        return f"block_edges {got['block_edges']}, reference {want['block_edges']}"
    for name, unit in (("roff", "position"), ("flags", "position"), ("codes", "slot")):
        g, w = np.asarray(got[name]), np.asarray(want[name])
        if g.shape != w.shape:
            return f"{name} has shape {g.shape}, reference {w.shape}"
        bad = np.flatnonzero(g != w)
        if len(bad):
            i = int(bad[0])
            where = ""
            if name == "codes":
                p = int(np.searchsorted(want["roff"], i, side="right")) - 1
                while want["lay"][p] == 0:       # (rows without codes share their successor's offset)
                    p += 1
                where = f" (position {p}, edge k = {i - int(want['roff'][p]) + 1} of {int(want['kend'][p])})"
            return f"{name} at {unit} {i}{where}: {int(g[i]):#x}, reference {int(w[i]):#x} ({len(bad)} differ)"
    for name in ("winflag", "winroff"):
        g, w = np.asarray(got[name]), np.asarray(want[name])
        if g.shape != w.shape:
            return f"{name} has shape {g.shape}, reference {w.shape}"
        bad = np.flatnonzero((g != w) & want["win_defined"])
        if len(bad):
            i = int(bad[0])
            return f"{name} of window {i}: {int(g[i]):#x}, reference {int(w[i]):#x} ({len(bad)} differ)"
    g, w = np.asarray(got["wmeta"]), want["wmeta"]
    if g.shape != w.shape:
        return f"wmeta has shape {g.shape}, reference {w.shape}"
    bad = np.argwhere((g != w) & want["wmeta_defined"])
    if len(bad):
        i, k = map(int, bad[0])
        return f"wmeta word {k} of window {i}: {int(g[i, k]):#x}, reference {int(w[i, k]):#x} ({len(bad)} differ)"
    return None


# ------------------------------------------------------------------------------------------------ GetBestLengths on the rows
def weight_table(ll, d):
    """The weight of every code, as the comment of k_wtab states it: 0 = no edge, 1 + byte = the literal's cost,
    257 + 30 (lsym - 257) + dsym = ((extra bits of both symbols) + ll[lsym]) + d[dsym] (squeeze.c:146-157)."""
    w = np.full(1152, np.inf)
    w[1:257] = np.asarray(ll, dtype=np.float64)[:256]
    for c in range(257, 1127):
        ls, ds = 257 + (c - 257) // 30, (c - 257) % 30
        lbits = 0 if ls < 265 or ls == 285 else (ls - 261) // 4         # RFC 1951, 3.2.5
        dbits = 0 if ds < 4 else ds // 2 - 1
        w[c] = (float(lbits + dbits) + float(ll[ls])) + float(d[ds])
    return w


def best_lengths(lay, ll, d, mincost):
    """GetBestLengths (squeeze.c:217-304) over the rows of a reference layout that holds codes for every row: an edge's
    cost is weight_table[code / 8].  -> length_array[0 .. B]."""
    B = len(lay["kend"])
    w = weight_table(ll, d)
    codes = lay["codes"].astype(np.int64) >> 3
    assert not lay["codeless"].any()
    roff, kend, shortcut = lay["roff"].astype(np.int64), lay["kend"].astype(np.int64), lay["shortcut"]
    costs = np.full(B + 1, 1e30, dtype=np.float32)
    costs[0] = 0
    la = np.zeros(B + 1, dtype=np.uint16)
    run258 = w[257 + 30 * (int(_LSYM[MAX_MATCH]) - 257) + 0]              # a match of 258 at distance 1
    j = 0
    while j < B:
        if shortcut[j]:                                                  # squeeze.c:251-271
            for _ in range(MAX_MATCH):
                costs[j + MAX_MATCH] = np.float32(np.float64(costs[j]) + run258)
                la[j + MAX_MATCH] = MAX_MATCH
                j += 1
        r, ke, cj = int(roff[j]), int(kend[j]), np.float64(costs[j])
        new = w[codes[r]] + cj                                           # squeeze.c:277-284
        if new < costs[j + 1]:
            costs[j + 1] = np.float32(new)
            la[j + 1] = 1
        if ke >= 3:                                                      # squeeze.c:286-302
            tgt = costs[j + 3:j + ke + 1]
            new = w[codes[r + 2:r + ke]] + cj
            take = (tgt.astype(np.float64) > mincost + cj) & (new < tgt)
            tgt[take] = new[take].astype(np.float32)
            la[j + 3:j + ke + 1][take] = np.arange(3, ke + 1, dtype=np.uint16)[take]
        j += 1
    return la


def fixed_tree_costs():
    """GetCostFixed (squeeze.c:112-133) as the ll / d arrays of a cost model: the code lengths of the fixed tree."""
    ll = np.array([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, dtype=np.float64)
    return ll, np.full(32, 5.0)


def subchunks(lay):
    """The stated packing rule of k_codes on a layout: within every group of 64 positions (aligned to the block start) a
    sub-chunk is the longest prefix of the rows not yet taken whose slots total at most EG_CAP.  -> [(first position,
    rows, slots)]."""
    n = np.asarray(lay["lay"], dtype=np.int64)
    out = []
    for base in range(0, len(n), 64):
        q, end = base, min(base + 64, len(n))
        while q < end:
            tot = np.cumsum(n[q:end])
            rows = int(np.searchsorted(tot, EG_CAP, side="right"))
            assert rows >= 1
            out.append((q, rows, int(tot[rows - 1])))
            q += rows
    return out


# ------------------------------------------------------------------------------------------------ planting
class Planter:
    """Random bytes (three equal bytes in a row some thousand positions apart are rare and harmless: the CPU test asserts
    what every case reaches) into which copies are planted; `used` keeps what a later plant must leave alone."""

    def __init__(self, n, seed):
        self.rng = np.random.default_rng(seed)
        self.a = self.rng.integers(0, 256, n, dtype=np.uint8)
        self.used = np.zeros(n, dtype=bool)

    def free(self, lo, hi):
        return lo >= 0 and hi <= len(self.a) and not self.used[lo:hi].any()

    def put(self, p, b):
        b = np.frombuffer(bytes(b), dtype=np.uint8)
        assert self.free(p, p + len(b)), p
        self.a[p:p + len(b)] = b
        self.used[p:p + len(b)] = True

    def periodic(self, p, n, pair):
        """n bytes of period 2 that the byte behind them does not continue."""
        self.put(p, (bytes(pair) * (n // 2 + 1))[:n])
        self.put(p + n, bytes([pair[n % 2] ^ 0x55]))

    def run(self, p, n, byte):
        """n equal bytes with other bytes on either side."""
        self.put(p - 1, bytes([byte ^ 0x55]))
        self.put(p, bytes([byte]) * n)
        if p + n < len(self.a):
            self.put(p + n, bytes([byte ^ 0x33]))

    def copy_at(self, p, L, D):
        """a[p : p + L] becomes a copy of what lies D before it (D < L: bytes of period D) that ends there."""
        a = self.a
        assert self.free(p, p + L + 1) and (D < L or self.free(p - D, p - D + L + 1)), (p, D)
        if a[p - D] == a[p - D + 1]:                 # (no run of equal bytes: a nearer copy of it would come first)
            a[p - D + 1] ^= 0x11
        for i in range(L):
            a[p + i] = a[p - D + i]
        a[p + L] = a[p - D + L] ^ 0x55
        self.used[max(p - D, 0):min(p - D + L + 1, p)] = True
        self.used[p:p + L + 1] = True

    def change_points(self, p, lengths):
        """Position p gets one change point per entry of `lengths` (ascending): a fresh string at p and, going back
        from p, a copy of its first l bytes for every l, nearer copies shorter; every copy ends in a byte that differs
        (a block end inside the string cuts the longer copies).  -> how far back the copies reach."""
        top = max(lengths)
        T = self.rng.integers(0, 256, top + 1, dtype=np.uint8)
        if T[0] == T[1]:
            T[1] ^= 0x11
        self.put(p, T[:top])
        src = p
        for l in lengths:
            src -= l + 1
            while not self.free(src, src + l + 1):
                src -= 1
            assert p - src < 32768, "the copies do not fit the window"
            self.put(src, bytes(T[:l]) + bytes([T[l] ^ 0x55]))
        return p - src

    def bytes(self):
        return self.a.tobytes()


class Case:
    def __init__(self, name, data, blocks, **marks):
        self.name, self.data, self.blocks, self.marks = name, data, blocks, marks


def _contiguous(start, sizes):
    blocks = []
    for n in sizes:
        blocks.append((start, start + n))
        start += n
    return blocks


SHAPE_SIZES = [0, 1, 2, 3, 63, 64, 65, 96, 97, 1023, 1024, 1025, 2047, 2048, 2049, 4096]
MAX_CPS = list(range(3, 255))       # 252 copies of 4 .. 255 bytes end 32 634 positions back: one more leaves the window
CP_COUNTS = (0, 1, 7, 8, 9, 16, len(MAX_CPS))


def _shapes():
    """Class T cut into blocks of the sizes at which the kernels take another step: 1024 (k_rowscan's carry), 2048
    (k_codes' tiles), 32 (k_mkdesc's windows), and the tiny ones."""
    blocks = _contiguous(300, SHAPE_SIZES)
    return Case("shapes", generate("T", blocks[-1][1] + 300), blocks)


def _multi():
    """Four blocks of class T in one table: an empty one in the middle, one with instart > 32768 (its own code_base,
    pos_off and win_off, and matches into the window at its first position).  MULTI_PARENT encloses them."""
    return Case("multi", generate("T", 45000), [(300, 5000), (5000, 5000), (5000, 9000), (40000, 44500)])


MULTI_PARENT = [(0, 45000)]


def _kend_cut():
    """Block 0 ends inside bytes of period 2 (one change point at distance 2: no run row), block 1 inside a run of equal
    bytes: over the last 260 positions kend falls 258, 258, 258, 257, .., 3, 1, 1."""
    p = Planter(3800, 11)
    p.periodic(300, 1400, b"ab")
    p.run(2000, 1500, 0x7a)
    return Case("kend_cut", p.bytes(), [(0, 1300), (1700, 2800)])


def _change_points():
    """Positions with exactly 1, 7, 8, 9, 16 and 252 change points (0: the random bytes around them), and near the ends
    of blocks 0 and 1 a pool record (16 planted) and an inline one (8 planted) whose longer copies the block end cuts."""
    N = 52000
    p = Planter(N, 12)
    at = {}
    at[len(MAX_CPS)] = 33000
    p.change_points(33000, MAX_CPS)
    cur = 33300
    for lengths in ([40], [3, 4, 10, 30, 31, 100, 258], [3, 5, 9, 17, 33, 65, 129, 257], [3, 4, 5, 6, 7, 8, 9, 10, 258],
                    list(range(3, 19))):
        cur += sum(l + 1 for l in lengths) + 8
        p.change_points(cur, lengths)
        at[len(lengths)] = cur
        cur += max(lengths) + 8
    # a pool record 40 positions before the end of block 0: copies of 3, 6, .., 48 bytes
    lengths = list(range(3, 49, 3))
    cur += sum(l + 1 for l in lengths) + 8
    e0 = cur + 40
    p.change_points(cur, lengths)
    cut_pool = cur
    cur = e0 + 60
    # an inline record 100 positions before the end of block 1
    lengths = [3, 5, 9, 17, 33, 65, 129, 200]
    cur += sum(l + 1 for l in lengths) + 8
    e1 = cur + 100
    p.change_points(cur, lengths)
    assert e1 + 300 < N
    return Case("change_points", p.bytes(), [(0, e0), (e0, e1), (e1, N)], at=at, cut_pool=(0, cut_pool, 16),
                cut_inline=(1, cur - e0, 8))


def _subchunks():
    """One block.  Rows of 258 slots (bytes of period 2), the ramp 257, 256, .. 3, 1, 1 where such bytes end, and
    literals (random bytes, one slot each) placed so that groups of 64 positions hold: 64 rows of 258 (group 384);
    258 x 3 + 257 + 256 + 255 + 254 = 1796 with the next row making 2049 (group 640); 20 + 19 + .. + 3, two literals,
    31 more, two more and 7 rows of 258 = 2048 exactly (group 1344), the same with 30 literals = 2047 (group 2368); a
    pool record as the first row of a sub-chunk (3200), as the last (3519), and two in one (3850, 3890)."""
    p = Planter(4300, 13)
    p.periodic(300, 600, b"ab")           # 258 up to position 642, then 257 at 643
    p.periodic(1000, 364, b"cd")          # kend 20 at position 1344
    p.periodic(1395, 600, b"ef")          # 1, 1, then 258 from 1397
    p.periodic(2100, 288, b"gh")          # kend 20 at position 2368
    p.periodic(2418, 600, b"ij")
    pool = [3200, 3519, 3850, 3890]
    for q in pool:
        p.change_points(q, list(range(3, 12)))
    return Case("subchunks", p.bytes(), [(0, 4300)], pool=pool,
                want={384: [(384 + 7 * i, 7, 1806) for i in range(9)] + [(447, 1, 258)],
                      640: (640, 7, 1796), 1344: (1344, 60, 2048), 2368: (2368, 59, 2047)})


def _symbols():
    """Every byte value as a literal, every length 3 .. 258 as an edge (bytes of period 2) and a planted copy of 6 bytes
    at the first and the last distance of every distance symbol."""
    N = 36000
    p = Planter(N, 14)
    p.put(100, bytes(range(256)))
    p.periodic(500, 400, b"ab")
    cur = 33000
    for D in dist_boundaries():
        while not (p.free(cur, cur + 7) and (D < 6 or p.free(cur - D, cur - D + 7))):
            cur += 1
        p.copy_at(cur, 6, D)
        cur += 16
    assert cur < N
    return Case("symbols", p.bytes(), [(0, N)])


def _shortcut():
    """Runs of equal bytes on the four inequalities of squeeze.c:251-258.  Block 0 (2800 positions) begins with a run of
    1400 (j = 259 | 260; its end: same = 517 | 516 at j = 882 | 883), a second run begins at its position 1700 (the
    run begins 257 | 258 positions before j = 1957 | 1958) and is cut by the block end (j + 517 = B - 1 | B at j =
    2282 | 2283: there same, counted inside the block, falls to 516 with it — the two cannot be told apart).  Block 1
    holds a run of 66 200 bytes: same is 65535 at both ends of the comparison."""
    p = Planter(70200, 15)
    p.run(500, 1400, 0x00)
    p.run(2200, 1300, 0xff)
    p.run(3700, 66200, 0x00)
    return Case("shortcut", p.bytes(), [(500, 3300), (3300, 70200)],
                flips={"j > 259": (0, 259, [1]), "same > 516 at the run's end": (0, 882, [0]),
                       "same[j - 258] > 258": (0, 1957, [3]), "j + 517 < B, the run cut by the block end": (0, 2282, [0, 2])})


def _not_run_rows():
    """Inside a short run a position whose longest match is a farther copy (two change points, best distance not 1), and
    a run of exactly 66 equal bytes: rows of 65, 64, 63, .. edges at distance 1, on either side of the codeless
    threshold."""
    p = Planter(900, 16)
    T = bytes([0x51, 0x52, 0x53, 0x54, 0x55])
    p.put(199, b"\x01" + b"\x40" * 6 + T + b"\x02")
    p.put(399, b"\x03" + b"\x40" * 6 + T + b"\x04")
    p.run(600, 66, 0x71)
    return Case("not_run_rows", p.bytes(), [(0, 900)], far=402, run66=600)


def _class(cls):
    return Case("class_" + cls, generate(cls, 70000), [(0, 70000)])


_BUILDERS = dict(shapes=_shapes, multi=_multi, kend_cut=_kend_cut, change_points=_change_points, subchunks=_subchunks,
                 symbols=_symbols, shortcut=_shortcut, not_run_rows=_not_run_rows,
                 class_T=lambda: _class("T"), class_Z=lambda: _class("Z"))
CASES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def layouts(name, codeless):
    """reference_layout of every block of the case."""
    c = case(name)
    return [reference_layout(c.data, s, e, codeless) for s, e in c.blocks]
