"""Inputs that put k_same and k_chain (zmx_kernels.h) where they decide something, and the plain reference of what
they build: same[], prev1[], prev2[] read out of the real reference's own hash state (hash.c:100-137), update by
update.  The synthetic classes never get there: their longest run is 5000 bytes, no two positions of one hash value lie
exactly a window apart with nothing of that value between them, and their last block ends where the input ends.

A "region" is what a block's hash arrays cover, windowstart .. inend - 1; a region index is a position minus
windowstart.  k_same works in stretches of 64 region indices (SAME_CH), k_chain in chunks of 32768 (CH_EMIT) that
warm up from the 32768 before them, 64 positions (one step) at a time.

Test infrastructure only: tests/test_cpu_hash_link_cases.py pins the oracle to the reference on these cases and
asserts that every case reaches what it is named for; tests/test_gpu_hash_link_edges.py runs the kernels on them."""
import ctypes
import functools

import numpy as np

import oracle_lib as ol

WINDOW = 32768
CAP = 65535           # hash.c:121-123: same[] is an unsigned short
STEP = 64             # positions per k_chain step, region indices per k_same thread
MT = 2048             # k_match2's tile: tables built from a parent recompute whole tiles


def windowstart(instart):
    return instart - WINDOW if instart > WINDOW else 0


# ---- the plain reference ----------------------------------------------------------------------------------------------
def reference_links(data, instart, inend):
    """(same, prev1, prev2) as uint16 arrays over windowstart .. inend - 1: ZopfliAllocHash, ZopfliResetHash,
    ZopfliWarmupHash(ws, inend), then ZopfliUpdateHash(p, inend) for every p, exactly as ZopfliLZ77Greedy drives them.
    After the update of p, with hpos = p & 32767: same[hpos], (hpos - prev[hpos]) & 32767, (hpos - prev2[hpos]) & 32767;
    prev[hpos] == hpos is the reference's "none" and gives 0, which is how lz77.c:521-523 treats it.

    An update writes slot hpos of the three arrays and no other slot, and the slot is written again only 32768
    positions later: the slots are copied out after every stretch of at most 32768 updates instead of one by one."""
    lib = ol.ref()
    ws = windowstart(instart)
    n = inend - ws
    out = [np.zeros(n, dtype=np.uint16) for _ in range(3)]
    if n == 0:
        return tuple(out)
    h = ol.RefHash()
    lib.ZopfliAllocHash(WINDOW, ctypes.byref(h))
    try:
        lib.ZopfliResetHash(WINDOW, ctypes.byref(h))
        lib.ZopfliWarmupHash(data, ws, inend, ctypes.byref(h))
        state = [np.ctypeslib.as_array(p, shape=(WINDOW,)) for p in (h.same, h.prev, h.prev2)]
        update, href = lib.ZopfliUpdateHash, ctypes.byref(h)
        for a in range(ws, inend, WINDOW):
            b = min(a + WINDOW, inend)
            for p in range(a, b):
                update(data, p, inend, href)
            hpos = np.arange(a, b, dtype=np.int64) & (WINDOW - 1)
            out[0][a - ws:b - ws] = state[0][hpos]
            for o, s in zip(out[1:], state[1:]):
                o[a - ws:b - ws] = (hpos - s[hpos].astype(np.int64)) & (WINDOW - 1)
    finally:
        lib.ZopfliCleanHash(ctypes.byref(h))
    return tuple(out)


def hash_values(data, ws, inend):
    """hash.c:96-98, 107-108 restated for the reach facts only: the first chain's key at ws .. inend - 1, zeros for the
    bytes at and past inend."""
    b = np.zeros(inend - ws + 2, dtype=np.int64)
    b[:inend - ws] = np.frombuffer(data, dtype=np.uint8, count=inend - ws, offset=ws)
    return ((b[:-2] << 10) ^ (b[1:-1] << 5) ^ b[2:]) & 32767


def _nearest_earlier(keys):
    """Distance to the nearest earlier index with the same key (0 = none), whatever the distance."""
    order = np.lexsort((np.arange(len(keys)), keys))
    d = np.zeros(len(keys), dtype=np.int64)
    eq = keys[order[1:]] == keys[order[:-1]]
    d[order[1:][eq]] = (order[1:] - order[:-1])[eq]
    return d


# ---- building blocks --------------------------------------------------------------------------------------------------
def _h3(a, b, c):
    return ((a << 10) ^ (b << 5) ^ c) & 32767


def _settle(rng, data, fixed, exempt, forbidden, lo=1):
    """Resample the bytes of `data` that are not `fixed` until no position outside `exempt` has a hash value in
    `forbidden` and no two neighbours are equal unless both are fixed (so that same[] is 0 wherever nothing was planted
    and the second chain's key is the first's ^ 253 there).  Fails if fixed bytes alone break a rule."""
    n = len(data)
    forb = np.zeros(32768, dtype=bool)
    for k in forbidden:
        forb[k] = True
    for _ in range(200):
        b = np.zeros(n + 2, dtype=np.int64)
        b[:n] = data
        val = ((b[:-2] << 10) ^ (b[1:-1] << 5) ^ b[2:]) & 32767
        bad = np.nonzero(forb[val] & ~exempt)[0]
        eq = np.nonzero((data[1:] == data[:-1]) & ~(fixed[1:] & fixed[:-1]))[0]
        if len(bad) == 0 and len(eq) == 0:
            return
        for i in bad:
            free = [j for j in range(i, min(i + 3, n)) if not fixed[j]]
            assert free, f"planted bytes alone give a forbidden hash value at {i}"
            data[free[int(rng.integers(len(free)))]] = rng.integers(lo, 256)
        for i in eq:
            j = i + 1 if not fixed[i + 1] else i
            data[j] = rng.integers(lo, 256)
    raise AssertionError("filler did not settle")


class Case:
    def __init__(self, name, data, blocks, **facts):
        self.name = name
        self.data = bytes(data)
        self.blocks = list(blocks)
        self.facts = facts      # what the builder planted, by region index or position (reach() checks it in the links)
        assert len(self.data) <= 200000

    def __repr__(self):
        return self.name


def _rand(rng, n, lo=0):
    return rng.integers(lo, 256, size=n, dtype=np.uint8)


def _glue(rng, parts):
    """Concatenate random stretches (ints: that many bytes) and runs ((symbol, length) pairs); the random byte on
    either side of a run differs from the run's symbol, so the run is exactly as long as it says."""
    out = []
    for i, p in enumerate(parts):
        if isinstance(p, tuple):
            out.append(np.full(p[1], p[0], dtype=np.uint8))
        else:
            r = _rand(rng, p)
            for nb, at in ((parts[i - 1] if i else None, 0), (parts[i + 1] if i + 1 < len(parts) else None, -1)):
                if isinstance(nb, tuple) and p:
                    while r[at] == nb[0]:
                        r[at] = rng.integers(0, 256)
            out.append(r)
    return np.concatenate(out)


# ---- run-cap ----------------------------------------------------------------------------------------------------------
def _run_cap_a():
    # following equal bytes: exactly 65534 (0x00) and exactly 65535 (0xff)
    rng = np.random.default_rng(6553401)
    data = _glue(rng, [301, (0x00, 65535), 203, (0xff, 65536), 157])
    n = len(data)
    return Case("run-cap-a", data, [(0, n)])               # one block: nothing but the cap bounds the runs


def _run_cap_b():
    # following equal bytes: exactly 65536 (0xff: 2 capped positions) and exactly 65537 (0x00: 3 of them)
    rng = np.random.default_rng(6553602)
    data = _glue(rng, [5, (0xff, 65537), 99, (0x00, 65538), 64])
    n = len(data)
    return Case("run-cap-b", data, [(0, n)])


RUN_C = dict(run0=(500, 100500), run1=(100800, 170800), n=175000)


def _run_cap_c_data():
    rng = np.random.default_rng(100000)
    data = _glue(rng, [500, (0x00, 100000), 300, (0xff, 70000), 4200])
    assert len(data) == RUN_C["n"]
    return data


def _run_cap_c():
    blocks = [
        (0, 60000),         # inend inside the 100000-byte run: the block end, not the cap, bounds same[] near it
        (60000, 110000),    # windowstart 27232 lies inside the capped part of that run; the run ends in the block
        (110000, 150000),   # the 0xff run starts in the window (100800) and runs through inend
        (150000, 175000),   # windowstart inside the 0xff run, which ends in the block; random bytes to the end
    ]
    return Case("run-cap-c", _run_cap_c_data(), blocks)


def _run_cap_d():
    # the same input as one block: the 100000-byte run whole, 34465 capped positions in a row
    return Case("run-cap-d", _run_cap_c_data(), [(0, RUN_C["n"])])


def _mixed_lengths():
    # one table set over blocks of very different L: grids sized for the longest, the `c0 >= L` and `e0 >= L` early
    # returns for the short and the empty ones
    n = RUN_C["n"]
    return Case("mixed-lengths", _run_cap_c_data(), [(0, 3), (3, 5), (5, 5), (5, 70000), (70000, n)])


# ---- run-scan ---------------------------------------------------------------------------------------------------------
SCAN_RES = [1, 2, 3, 4, 5, 6, 7, 0, 3, 6]     # (cut - 32768) % 8 = the next block's windowstart % 8


def _run_scan():
    rng = np.random.default_rng(6408)
    cuts = [WINDOW + 8 * (30 + 313 * i) + r for i, r in enumerate(SCAN_RES)]
    n = cuts[-1] + 2000
    data = _rand(rng, n)
    fixed = np.zeros(n, dtype=bool)

    def plant(start, length, sym=None):
        """A run of exactly `length` bytes at `start`."""
        if sym is None:
            sym = int(rng.integers(0, 256))
        data[start:start + length] = sym
        fixed[start:start + length] = True
        for j in (start - 1, start + length):
            if 0 <= j < n and not fixed[j]:
                while data[j] == sym:
                    data[j] = rng.integers(0, 256)
        return sym

    # every (start offset mod 8, r) pair: runs of 64 k + r bytes, k = 1 or 2, below the first cut, so that the first
    # block and every later block's window see them all
    pos = 3
    k = 0
    for r in range(24):
        for off in range(8):
            pos += (off - pos) % 8 or 8
            length = 64 * (1 + k % 2) + r
            k += 1
            plant(pos, length)
            pos += length + 1
    assert pos < cuts[0] - 200, pos
    # the block ends: the first differing byte at inend - 1 - j for j = 0 .. 8 (cuts 0 .. 8), a run cut by inend itself
    # (cut 9) and a run through the input's end
    for j, c in enumerate(cuts[:9]):
        plant(c - 1 - j - 70, 70)
    plant(cuts[9] - 40, 90)
    plant(n - 75, 75)
    # runs whose first differing byte is one before, on and one after a multiple of 64 from windowstart, in every block
    # that has a windowstart of its own
    for i, c in enumerate(cuts):
        ws = c - WINDOW
        m0 = (c + 300 - ws) // 64 + 1
        for t, delta in enumerate((-1, 0, 1)):
            end = ws + 64 * (m0 + 3 * t) + delta
            plant(end - 67, 67)
    # no equal neighbours left in the filler: the runs are exactly the planted ones
    _settle(rng, data, fixed, np.ones(n, dtype=bool), [], lo=0)
    blocks = [(0, cuts[0])] + [(cuts[i], cuts[i + 1]) for i in range(9)] + [(cuts[9], n)]
    return Case("run-scan", data, blocks)


# ---- window-edge ------------------------------------------------------------------------------------------------------
def _edge_input(seed, ws, length, tris=(), fives=(), runs=(), tail=0):
    """`ws` bytes, then a region of `length` bytes (region index r = position ws + r), then `tail` bytes.
    tris:  (r, d)  a 3-byte marker at r and again at r + d: one hash value, at two positions d apart.
    fives: (r, d)  a 5-byte marker: three consecutive positions, each d after its twin.
    runs:  (r, d, m1, m2)  a run of m1 equal bytes at r and one of m2 of the same symbol at r + d (4 .. 10 bytes: same[]
           is at least 3 at the start, and the second chain's key is not the first's).
    The filler holds none of the markers' hash values on either chain and no two equal neighbours."""
    rng = np.random.default_rng(seed)
    n = ws + length + tail
    data = _rand(rng, n)
    fixed = np.zeros(n, dtype=bool)
    exempt = np.zeros(n, dtype=bool)
    forbidden = set()
    syms = list(rng.permutation(256))

    def put(r, b, nkeys):
        p = ws + r
        assert not fixed[max(p - 1, 0):p + len(b) + 1].any(), f"markers touch at region index {r}"
        data[p:p + len(b)] = b
        fixed[p:p + len(b)] = True
        exempt[p:p + nkeys] = True

    for group, size in ((tris, 3), (fives, 5)):
        for r, d in group:
            while True:
                b = rng.integers(1, 256, size=size)
                keys = {_h3(*b[i:i + 3]) for i in range(size - 2)}
                if len(set(b)) == size and len(keys) == size - 2 and not (keys & forbidden):
                    break
            forbidden |= keys
            put(r, b, size - 2)
            put(r + d, b, size - 2)
    for r, d, m1, m2 in runs:
        while True:
            a = int(syms.pop())
            ka = _h3(a, a, a)
            keys = {ka} | {ka ^ 253 ^ ((s - 3) & 255) for s in range(0, 10)}
            if not (keys & forbidden):
                break
        forbidden |= keys
        put(r, [a] * m1, m1 - 2)
        put(r + d, [a] * m2, m2 - 2)
    _settle(rng, data, fixed, exempt, forbidden)
    return data


EDGE_A = dict(ws=237, length=103000,
              fives=[(32769, 32766)],               # 65535 (with its twin inside chunk 1), 65536 and 65537 (across)
              tris=[(100, 32767), (110, 32768), (120, 32769), (130, 32766),      # across the seam at 32768
                    (32900, 32767), (32910, 32768), (32920, 32769), (32930, 32766),  # across the seam at 65536
                    (65600, 32767), (65610, 32768)])                      # into the last, partial chunk
EDGE_B = dict(ws=1, length=103000,
              tris=[(32768, 32767),                 # a chunk's first and last position: 65535 links 32767 back
                    (6, 32768), (12, 32769),        # second marker just after the seam, its twin just after w0
                    (32790, 32768), (32796, 32769), (32810, 32766),    # the same at the seam at 65536
                    (65542, 32767), (65550, 32766)])                   # into the last, partial chunk
EDGE_RUNS = dict(ws=237, length=103000,
                 runs=[(32768, 32767, 7, 7),        # equal runs: the second starts at 65535 and crosses the seam
                       (200, 32767, 6, 6),          # equal same 32767 apart
                       (400, 32767, 5, 9), (500, 32767, 9, 5),   # different same 32767 apart
                       (600, 32768, 5, 5), (700, 32769, 4, 4), (800, 32766, 8, 8),
                       (33000, 32768, 10, 10), (33100, 32766, 4, 4)])


def _edge_case(name, spec):
    ws, length = spec["ws"], spec["length"]
    data = _edge_input(sum(map(ord, name)), ws, length, spec.get("tris", ()), spec.get("fives", ()),
                       spec.get("runs", ()))
    # one block whose windowstart is `ws`: the region indices above are k_chain's own (chunks of 32768 from ws)
    pairs = [(0, r + i, d) for r, d in spec.get("fives", ()) for i in range(3)]
    pairs += [(0, r, d) for r, d in spec.get("tris", ())]
    run_pairs = [(0, r, d) for r, d, m1, m2 in spec.get("runs", ()) if m1 == m2]
    return Case(name, data, [(ws + WINDOW, ws + length)], pairs=pairs, run_pairs=run_pairs)


EDGE_ENDS = [(100, 32766), (110, 32767), (120, 32768), (130, 32769)]   # (windowstart, d)


def _edge_ends():
    # the first marker at region index 0 and the last at the block's last full position (inend - 3): blocks of 1, 2, 3
    # and 4 bytes with a whole window before them
    data = _rand(np.random.default_rng(1), 40000)
    n = len(data)
    rng = np.random.default_rng(32767)
    fixed = np.zeros(n, dtype=bool)
    exempt = np.zeros(n, dtype=bool)
    forbidden = set()
    for ws, d in EDGE_ENDS:
        while True:
            b = rng.integers(1, 256, size=3)
            k = _h3(*b)
            if len(set(b)) == 3 and k not in forbidden:
                break
        forbidden.add(k)
        for p in (ws, ws + d):
            data[p:p + 3] = b
            fixed[p:p + 3] = True
            exempt[p] = True
    _settle(rng, data, fixed, exempt, forbidden)
    blocks = [(ws + WINDOW, ws + d + 3) for ws, d in EDGE_ENDS]
    return Case("window-edge-ends", data, blocks, pairs=[(b, 0, d) for b, (_, d) in enumerate(EDGE_ENDS)])


# ---- step-groups ------------------------------------------------------------------------------------------------------
def _step_groups():
    rng = np.random.default_rng(64)
    seg = 33000
    parts = []
    for p in (1, 2, 3, 7, 64):
        unit = rng.permutation(256)[:p].astype(np.uint8)     # distinct bytes: the period is exactly p
        parts.append(np.tile(unit, seg // p + 1)[:seg])
    data = np.concatenate(parts)
    n = len(data)
    blocks = [
        (0, 70001),     # L = 70001: seams at 32768 (period 1) and 65536 (period 2)
        (70001, n),     # windowstart 37233, L = 127767: seams at 70001 (period 3), 102769 (period 7), 135537 (period 64)
    ]
    return Case("step-groups", data, blocks)


# ---- block-end-zeros --------------------------------------------------------------------------------------------------
ZERO_BLOCKS = [
    (0, 20011),         # plant 700 bytes before the end, no window
    (20011, 70002),     # windowstart 0, plant 30000 bytes before the end: inside the block
    (70002, 90003),     # windowstart 37234, plant in the window before instart (69000)
]
ZERO_PLANTS = [19311, 40002, 69000]


def _block_end_zeros():
    rng = np.random.default_rng(20011)
    n = 95000
    data = _rand(rng, n, lo=1)                   # no zero byte but the planted ones; non-zero bytes after every inend
    fixed = np.zeros(n, dtype=bool)
    exempt = np.zeros(n, dtype=bool)
    forbidden = set()
    for (s, e), at in zip(ZERO_BLOCKS, ZERO_PLANTS):
        while True:
            p, q, x, y = (int(v) for v in rng.integers(8, 256, size=4))
            keys = {_h3(p, q, 0), _h3(q, 0, 0), _h3(p, q, x), _h3(q, x, y)}
            if len({p, q, x, y}) == 4 and len(keys) == 4 and not (keys & forbidden):
                break
        forbidden |= keys
        data[at:at + 4] = (p, q, 0, 0)           # `p q 0` at `at`, `q 0 0` at `at + 1`
        data[e - 2:e + 2] = (p, q, x, y)         # the block ends `p q`, the input goes on `x y`
        fixed[at:at + 4] = True
        fixed[e - 2:e + 2] = True
        exempt[at:at + 2] = True
        exempt[e - 2:e] = True
    _settle(rng, data, fixed, exempt, forbidden)
    return Case("block-end-zeros", data, ZERO_BLOCKS, plants=ZERO_PLANTS)


_BUILDERS = {
    "run-cap-a": _run_cap_a, "run-cap-b": _run_cap_b, "run-cap-c": _run_cap_c, "run-cap-d": _run_cap_d,
    "run-scan": _run_scan,
    "window-edge-a": lambda: _edge_case("window-edge-a", EDGE_A),
    "window-edge-b": lambda: _edge_case("window-edge-b", EDGE_B),
    "window-edge-runs": lambda: _edge_case("window-edge-runs", EDGE_RUNS),
    "window-edge-ends": _edge_ends,
    "step-groups": _step_groups,
    "block-end-zeros": _block_end_zeros,
    "mixed-lengths": _mixed_lengths,
}
CASES = list(_BUILDERS)
FAMILIES = {"run-cap": ["run-cap-a", "run-cap-b", "run-cap-c", "run-cap-d"], "run-scan": ["run-scan"],
            "window-edge": ["window-edge-a", "window-edge-b", "window-edge-runs", "window-edge-ends"],
            "step-groups": ["step-groups"], "block-end-zeros": ["block-end-zeros"], "mixed-lengths": ["mixed-lengths"]}
MATCH_CASES = FAMILIES["run-cap"] + FAMILIES["window-edge"] + ["block-end-zeros", "step-groups"]


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def links(name, block):
    """reference_links of one block of a case, computed once and shared (read only)."""
    c = case(name)
    out = reference_links(c.data, *c.blocks[block])
    for a in out:
        a.setflags(write=False)
    return out


# ---- reuse: sub-blocks of a parent (0, n) over run-cap-c's input ------------------------------------------------------
_R0, _R1 = RUN_C["run0"][0], RUN_C["run1"][0]
REUSE_SUBBLOCKS = {
    "ends-in-run": [
        (0, _R0 + 3 * MT - 1),                  # ends inside the 100000-byte run, MT k - 1 after its start
        (_R0 + 3 * MT - 1, _R0 + 10 * MT),      # ... MT k after it: the whole sub-block is run
        (_R0 + 10 * MT, _R0 + 20 * MT + 1),     # ... MT k + 1
        (_R0 + 20 * MT + 1, _R0 + 20 * MT + 301),   # 300 bytes inside the run
        (_R0 + 20 * MT + 301, RUN_C["run0"][1] + 1),   # ends one byte after the run's end
        (RUN_C["run0"][1] + 1, 140000),         # ends inside the 0xff run, which began in this sub-block
        (140000, 165000),                       # one run from before its windowstart (107232) to its inend
        (165000, RUN_C["n"]),                   # same end as the parent: every record is the parent's
    ],
    "skips-chunks": [
        (0, _R1 + 14 * MT),                     # the tail run starts 100800 in: link_lo = 67584, k_chain skips two
        (_R1 + 14 * MT, RUN_C["n"]),            # chunks and k_same what lies below the third's warm-up
    ],
}


# ---- what the cases reach, from the reference's links -----------------------------------------------------------------
def _stretches(mask):
    """Lengths of the maximal stretches of True."""
    m = np.concatenate(([0], mask.astype(np.int8), [0]))
    d = np.diff(m)
    return (np.nonzero(d == -1)[0] - np.nonzero(d == 1)[0]).tolist()


def reach(name):
    """Facts about one case, read from reference_links (and, for the keys, hash_values of the input): the CPU test
    asserts on them, family by family."""
    c = case(name)
    f = dict(capped_stretches=[], run_start_same=set(), uniform_step2=0, scan_pairs=set(), ws_mod8=set(),
             end_j=set(), cut_by_inend=0, end_mod64={}, links={1: set(), 2: set()}, zero_at={1: set(), 2: set()},
             pairs={}, run_pairs={}, warm_group=0, emit_group=0, end_links=[])
    for b, (s, e) in enumerate(c.blocks):
        if e == s:
            continue
        ws = windowstart(s)
        same, prev1, prev2 = (a.astype(np.int64) for a in links(name, b))
        n = e - ws
        val = hash_values(c.data, ws, e)
        key = {1: val, 2: val ^ ((same - 3) & 255)}
        prev = {1: prev1, 2: prev2}
        # runs, as same[] shows them: a run starts where the position before it has same == 0
        starts = np.nonzero((same > 0) & np.concatenate(([True], same[:-1] == 0)))[0]
        f["capped_stretches"] += _stretches(same == CAP)
        f["run_start_same"] |= set(same[starts].tolist()) & {CAP - 1, CAP}
        k2 = key[2][:n // STEP * STEP].reshape(-1, STEP)
        f["uniform_step2"] += int((k2 == k2[:, :1]).all(axis=1).sum())
        for i in starts.tolist():
            length = int(same[i]) + 1
            if i + length < n and length >= STEP:
                f["scan_pairs"].add(((ws + i) % 8, (length - STEP) % STEP))
            if i + length == n:
                f["cut_by_inend"] += 1
            elif n - 1 - (i + length) <= 8:
                f["end_j"].add(n - 1 - (i + length))
            if ws:
                f["end_mod64"].setdefault(b, set()).add((i + length) % STEP)
        f["ws_mod8"].add(ws % 8)
        for ch in (1, 2):
            true_d = _nearest_earlier(key[ch])
            # the links are the nearest earlier position of the key when that is at most 32767 back, else none
            assert np.array_equal(prev[ch], np.where(true_d <= WINDOW - 1, true_d, 0)), (name, b, ch)
            f["links"][ch] |= set(prev[ch][prev[ch] >= WINDOW - 2].tolist())
            f["zero_at"][ch] |= set(true_d[(prev[ch] == 0) & (true_d > 0) & (true_d <= WINDOW + 1)].tolist())
        # what was planted as (block, region index, d): the true distance to the key's nearest earlier position on
        # either chain, and the two links, at region index r + d
        for kind in ("pairs", "run_pairs"):
            for pb, r, d in c.facts.get(kind, ()):
                if pb == b:
                    i = r + d
                    f[kind][(b, r, d)] = (int(_nearest_earlier(key[1])[i]), int(_nearest_earlier(key[2])[i]),
                                          int(prev1[i]), int(prev2[i]), int(same[i]))
        # steps of 64 region indices: below the last chunk's first position every step is a warm-up step of the chunk
        # after it; every step is an emit step of its own chunk
        last_e0 = (n - 1) // WINDOW * WINDOW
        for ch in (1, 2):
            ks = np.sort(key[ch][:n // STEP * STEP].reshape(-1, STEP), axis=1)
            run = np.ones(len(ks), dtype=np.int64)
            best = np.ones(len(ks), dtype=np.int64)
            for j in range(1, STEP):
                run = np.where(ks[:, j] == ks[:, j - 1], run + 1, 1)
                best = np.maximum(best, run)
            if len(best):
                f["emit_group"] = max(f["emit_group"], int(best.max()))
            if last_e0:
                f["warm_group"] = max(f["warm_group"], int(best[:last_e0 // STEP].max()))
        f["end_links"].append((b, int(prev1[n - 2]) if n >= 2 else 0, int(prev1[n - 1])))
    return f
