"""The cases of tests/test_cpu_png_lodeflate_seams.py and tests/test_gpu_png_lodeflate_seams.py: buffers built to put the
tile logic of zopfli_amd/csrc/device/zmx_png_lodeflate.h to work — links that ask several tables back, links that keep
what the slot held through several windows and tiles, zero-run keys over seams, tiles and chunks of one position, one
buffer behind another in a call, a lazy match over the parse's refill — at short tile lengths and at windows on both
sides of 8192.  A case is the buffers of ONE call (mostly one), the (window, tile length) pairs it runs at, and a `fact`:
a function that asserts, from the bytes alone, that the case reaches what it is there for.

In the facts, H is LodePNG's 16-bit hash of three bytes (its short form in a deflate block's last two positions), Z the
zero run LodePNG keeps beside it (0 where H is not 0), and "the previous equal position" the last earlier position of
the buffer with the same key, however far back."""
import functools

import numpy as np

import png_trial_cases as tc

WINDOWS = (256, 1024, 4096, 8192, 32768)
TILES = (255, 256, 257, 1000, 4096, 0)     # 0: the device's own
DEVICE_TILE = 262144
CHUNK = 256                                # k_png_lo_links walks a tile 256 positions at a time
PARSE_CHUNK = 2048                         # k_png_lo_parse stages 2048 positions at a time
MAX_BYTES, MAX_TILES = 140000, 600


# ---- what numpy makes of the bytes
def hashes(a):
    """H at every position of a buffer."""
    n = len(a)
    b = np.concatenate([a.astype(np.uint32), np.zeros(2, dtype=np.uint32)])
    p = np.arange(n, dtype=np.int64)
    bs = tc.blocksize(n)
    end = np.minimum((p // bs + 1) * bs, n)
    full = b[:n] ^ (b[1:n + 1] << 4) ^ (b[2:n + 2] << 8)
    short = b[:n] ^ np.where(p + 1 < end, b[1:n + 1] << 8, 0)
    return (np.where(p + 2 < end, full, short) & 65535).astype(np.int64)


def zero_runs(a):
    """Z at every position: where H is 0, the zeros from there on, at most 258 and not beyond the deflate block."""
    n = len(a)
    p = np.arange(n, dtype=np.int64)
    nxt = np.where(a != 0, p, n)
    nxt = np.minimum.accumulate(nxt[::-1])[::-1]          # the next byte that is not 0
    bs = tc.blocksize(n)
    end = np.minimum((p // bs + 1) * bs, n)
    z = np.minimum(np.minimum(nxt, end) - p, 258)
    return np.where(hashes(a) == 0, z, 0).astype(np.int64)


def trigrams(a):
    """The three bytes at every position but the last two, as one number."""
    b = a.astype(np.int64)
    return b[:-2] | (b[1:-1] << 8) | (b[2:] << 16)


def prev_equal(keys):
    """For every position the last earlier one with the same key, -1 where there is none."""
    keys = np.asarray(keys)
    order = np.argsort(keys, kind="stable")
    prev = np.full(len(keys), -1, dtype=np.int64)
    same = keys[order[1:]] == keys[order[:-1]]
    prev[order[1:][same]] = order[:-1][same]
    return prev


def links(keys, window):
    """What inserting every position writes into its slot p & (window - 1) of LodePNG's chain (its chainz, for Z): the slot
    of the previous equal position; where the key was never seen, what the slot held, which is what position p - window
    wrote, down to the slot's own number (LodePNG's "uninitialised")."""
    n = len(keys)
    prev = prev_equal(keys)
    c = np.where(prev >= 0, prev & (window - 1), -1)
    for s in range(0, n, window):
        e = min(n, s + window)
        held = np.arange(e - s) if s == 0 else c[s - window:e - window]
        c[s:e] = np.where(c[s:e] >= 0, c[s:e], held)
    return c


def model_words(a, window):
    """HC and ZC of a buffer as zmx_png_lodeflate.h defines them, from the bytes: H << 16 | C and Z << 16 | CZ."""
    h, z = hashes(a), zero_runs(a)
    return ((h << 16) | links(h, window)).astype(np.uint32), ((z << 16) | links(z, window)).astype(np.uint32)


def exact_zero_run(a, start, length):
    """The zeros of a[start : start + length] are a whole run: a byte that is not 0 on either side."""
    return (not a[start:start + length].any()) and a[start - 1] != 0 and a[start + length] != 0


def longest(a, pos, end, window):
    """tests/test_cpu_png_trial_cases.py's _longest: (length, distance) of the longest match at pos by plain comparison,
    the nearest of the longest, within the window and not beyond `end`."""
    best = (0, 0)
    for q in range(pos - 1, max(-1, pos - window - 1), -1):
        k = 0
        while pos + k < end and k < 258 and a[q + k] == a[pos + k]:
            k += 1
        if k > best[0]:
            best = (k, pos - q)
    return best


# ---- generators
def _rng(name):
    return np.random.default_rng(sum(ord(c) * (i + 1) for i, c in enumerate(name)) + 977)


@functools.lru_cache(maxsize=None)
def _no_repeat(n, span=256, seed=1):
    """`n` bytes below `span` in which no H occurs twice and none is 0: every byte is the first of a seeded stream of
    proposals whose trigram's hash is still free.  (tests/png_trial_cases.py's arithmetic sequence repeats its hashes
    every 251 positions, so it cannot serve where a key must never have been seen.)"""
    r = np.random.default_rng(seed)
    out = [int(v) for v in r.integers(0, span, 2)]
    used = bytearray(65536)
    used[0] = 1
    proposals = r.integers(0, span, 8 * n).tolist()
    at = 0
    while len(out) < n:
        low = out[-2] ^ (out[-1] << 4)
        for _ in range(64):
            v = proposals[at % len(proposals)]
            at += 1
            if not used[(low ^ (v << 8)) & 65535]:
                break
        else:
            v = next(v for v in range(span) if not used[(low ^ (v << 8)) & 65535])
        used[(low ^ (v << 8)) & 65535] = 1
        out.append(v)
    return np.array(out[:n], dtype=np.uint8)


class Case:
    def __init__(self, name, make, runs, fact, what):
        self.name, self._make, self.runs, self.fact, self.what = name, make, list(runs), fact, what

    @functools.lru_cache(maxsize=None)
    def bufs(self):
        """The buffers of the call (read-only)."""
        out = [np.ascontiguousarray(b, dtype=np.uint8) for b in self._make()]
        for b in out:
            b.setflags(write=False)
        return out

    @property
    def windows(self):
        return sorted({w for w, _ in self.runs})

    def check(self):
        bufs = self.bufs()
        for w, t in self.runs:
            assert w in WINDOWS, (self.name, w)
            for b in bufs:
                assert 0 < len(b) <= MAX_BYTES and -(-len(b) // (t or DEVICE_TILE)) <= MAX_TILES, (self.name, len(b), t)
        self.fact(bufs)


CASES = {}


def _add(name, make, runs, fact, what):
    assert name not in CASES
    CASES[name] = Case(name, make, runs, fact, what)


# ---- far-key: the previous position of a key lies k tiles back, inside the window and outside it
MARKER = (250, 251, 252)


def _far_key(name, k, tile):
    a = tc._noise(name, 10 + k * tile + 5 + 40, 250)
    a[10:13] = MARKER
    a[10 + k * tile + 5:10 + k * tile + 8] = MARKER
    return a


def _far_key_fact(k, tile, held, lost):
    def fact(bufs):
        a, = bufs
        p = 10 + k * tile + 5
        h = hashes(a)
        assert prev_equal(h)[p] == 10 and prev_equal(h)[10] == -1     # the marker's hash occurs there and nowhere else
        assert p // tile - 10 // tile == k and p % tile == 15
        assert p - 10 < held and p - 10 > lost                        # one window still holds position 10, one does not
    return fact


for _k, _tile, _held, _lost in ((1, 1000, 4096, 256), (2, 257, 1024, 256), (7, 4096, 32768, 8192)):
    _add(f"far-key-{_k}", functools.partial(lambda k, t: [_far_key(f"far-key-{k}", k, t)], _k, _tile),
         [(_held, _tile), (_lost, _tile), (_lost, 0)], _far_key_fact(_k, _tile, _held, _lost),
         f"LoAskWalk finds its key {_k} tables back; at window {_lost} the link is the stale slot LodePNG reads too")


# ---- never-seen: no key occurs twice, so every link keeps what its slot held, down to the slot itself
def _never_seen_fact(window, tile):
    def fact(bufs):
        a, = bufs
        n = len(a)
        h = hashes(a)
        first = prev_equal(h) == -1
        assert first[:n - 2].all()                                    # no H occurs twice (the end's two short ones aside)
        assert not (h[:n - 2] == 0).any()
        p = np.arange(2 * window, n)
        chained = first[p] & first[p - window] & first[p - 2 * window]
        # a walk through words that are KEEPs themselves, each in another tile than the last: every position from 2 W on,
        # which is a thousand of them wherever the buffer has as many
        assert chained.sum() >= n - 2 * window - 2 and window % tile == 0 and window // tile == 4
        assert chained.sum() >= (1000 if n > 5 * window + 3 else 3 * window)
    return fact


for _w in (256, 1024, 4096, 8192):
    _add(f"never-seen-{_w}", functools.partial(lambda w: [_no_repeat(5 * 8192 + 3)[:5 * w + 3]], _w), [(_w, _w // 4)],
         _never_seen_fact(_w, _w // 4), "every link is a KEEP whose walk takes up to 5 steps through KEEPs in other tiles")
# 5 * 256 + 3 bytes have 771 positions from 2 W on; the thousand positions whose p - W and p - 2 W are first occurrences
# as well are those of a longer stretch of the same bytes at window 256: walks of up to 80 steps over 321 tiles
_add("never-seen-256-long", lambda: [_no_repeat(5 * 8192 + 3)[:5 * 4096 + 3]], [(256, 64)], _never_seen_fact(256, 64),
     "at least 1000 KEEPs at window 256 whose p - W and p - 2 W are KEEPs too")


# ---- zero-runs-over-seams
ZERO_RUNS = (1, 2, 3, 257, 258, 259, 300)
ZERO_TILES = (256, 1000, 4096)


def _zero_plants():
    """(start, length) of the planted runs: for every tile length one run of every length over a seam of its own (a run
    of 1 ends a tile), and one of 300 over the block end at 65536."""
    plants = []
    for tile, first_seam, step in ((1000, 3000, 3000), (256, 256 * 100, 256 * 5), (4096, 4096 * 9, 4096)):
        for i, length in enumerate(ZERO_RUNS):
            seam = first_seam + i * step
            plants.append((seam - max(1, length // 2), length))
    plants.append((65536 - 140, 300))
    return plants


def _zero_runs_over_seams():
    a = tc._zero_heavy("zero-runs-over-seams", 70000, 0.5)
    for start, length in _zero_plants():
        a[start - 1] = 9
        a[start:start + length] = 0
        a[start + length] = 9
    return [a]


def _zero_runs_fact(bufs):
    a, = bufs
    assert tc.blocksize(len(a)) == 65536 and len(a) > 65536
    plants = _zero_plants()
    for start, length in plants:
        assert exact_zero_run(a, start, length), (start, length)
    for tile in ZERO_TILES:
        for length in ZERO_RUNS:
            over = [s for s, ln in plants if ln == length and (s // tile != (s + ln - 1) // tile if ln > 1 else s % tile == tile - 1)]
            assert over, (tile, length)
    assert any(s < 65536 < s + ln for s, ln in plants)
    z = zero_runs(a)
    pz = prev_equal(z)
    p = np.arange(len(a))
    assert z[65536 - 140] == 140 and z[65536] == 160                  # the run ends with the block and starts again
    for tile in ZERO_TILES:
        far = (z >= 3) & (pz >= 0) & (p // tile - pz // tile >= 3)
        assert far.any(), tile                                        # a Z whose previous position is three tiles back


_add("zero-runs-over-seams", _zero_runs_over_seams, [(256, 256), (1024, 1000), (8192, 1000), (4096, 4096), (8192, 0)], _zero_runs_fact,
     "zero runs of 1 .. 300 over tile seams and over the block end; zero-run keys that ask three tables back")


# ---- tile-len-edges: a last tile of one position, a last chunk of one live lane
def _mixed_bytes(name, n):
    """Zero-heavy bytes, filtered rows and noise over few values, with copies of earlier stretches."""
    r = _rng(name)
    parts, have = [], 0
    while have < n:
        m = int(r.integers(50, 900))
        kind = int(r.integers(0, 5))
        if kind == 0:
            part = tc._zero_heavy(f"{name}{have}", m, 0.3)
        elif kind == 1:
            part = tc._rows_like(f"{name}{have}", m)
        elif kind == 2:
            part = tc._noise(f"{name}{have}", m, 6)
        elif kind == 3:
            part = np.zeros(m, dtype=np.uint8)
        else:
            whole = np.concatenate(parts) if parts else tc._noise(name, m)
            s = int(r.integers(0, len(whole)))
            part = whole[s:s + m]
        parts.append(np.asarray(part, dtype=np.uint8))
        have += len(part)
    return np.concatenate(parts)[:n]


def _edge_fact(tile, n):
    def fact(bufs):
        a, = bufs
        assert len(a) == n and n - 3 * tile in (-1, 0, 1)
        lens = [tile] * (n // tile) + ([n % tile] if n % tile else [])
        assert (lens[-1] == 1) == (n == 3 * tile + 1) and (lens[-1] == tile - 1) == (n == 3 * tile - 1)
        assert any(ln % CHUNK == 1 for ln in lens) == (tile == 257 or n == 3 * tile + 1)    # a chunk of one live lane
        assert zero_runs(a).max() >= 3 and (prev_equal(hashes(a)) >= 0).any()
    return fact


for _tile in (255, 256, 257, 1000):
    for _n in (3 * _tile - 1, 3 * _tile, 3 * _tile + 1):
        _add(f"tile-len-edges-{_tile}-{_n}", functools.partial(lambda n: [_mixed_bytes(f"edges{n}", n)], _n), [(1024, _tile), (8192, _tile)],
             _edge_fact(_tile, _n), "tiles that end one short of, at and one beyond the buffer's end")


# ---- same-bytes-twice: [A, A, B, A] in one call
def _same_bytes_twice():
    a = _mixed_bytes("same-bytes-A", 9001)
    b = np.concatenate([a[100:400], tc._noise("same-bytes-B", 8200, 250) | 1])
    return [a, a.copy(), b, a.copy()]


def _same_bytes_fact(bufs):
    a, a2, b, a3 = bufs
    assert np.array_equal(a, a2) and np.array_equal(a, a3) and not np.array_equal(a[:len(b)], b[:len(a)])
    assert min(len(a), len(b)) > 2 * 4096                             # several tiles at every tile length of the case
    ha, hb = hashes(a), hashes(b)
    fresh = (prev_equal(hb)[:1000] == -1) & np.isin(hb[:1000], ha)
    assert fresh.sum() >= 100                                         # keys B has not seen yet and A's tables hold


_add("same-bytes-twice", _same_bytes_twice, [(256, 255), (1024, 1000), (8192, 4096), (8192, 0)], _same_bytes_fact,
     "first_tile: a buffer's links never look into the tables of the buffer in front of it")


# ---- block-and-tile-ends: a copy and a zero run over 65536, which is a seam at 4096 and inside a tile at 1000
def _block_and_tile_ends():
    a = tc._noise("block-and-tile-ends", 70000).copy()
    a[a == 0] = 1
    a[50150:50250] = 0
    a[65536 - 200:65536 + 200] = a[50000:50400]
    return [a]


def _block_ends_fact(bufs):
    a, = bufs
    assert len(a) == 70000 and tc.blocksize(len(a)) == 65536
    assert np.array_equal(a[65336:65736], a[50000:50400]) and exact_zero_run(a, 65486, 100)
    assert 65536 % 4096 == 0 and 0 < 65536 % 1000
    z = zero_runs(a)
    assert z[65486] == 50 and z[65536] == 50 and z[50150] == 100      # the run stops at the block's end and starts again


_add("block-and-tile-ends", _block_and_tile_ends, [(32768, 4096), (32768, 1000), (8192, 4096), (8192, 1000)], _block_ends_fact,
     "a block end on a seam and inside a tile, under a copy and a zero run")


# ---- parse-refill: a lazy match held, beaten, taken or jumped over where k_png_lo_parse refills its staged chunk
REFILL_X = (2045, 2046, 2047, 2048, 2049)
REFILL_OUTCOMES = ("beaten", "taken", "jump-258")
_M = (250, 251, 252, 253, 254, 255, 250, 252)       # no trigram twice; the bytes around them stay below 250
REFILL_QUIET = 600                                  # from here to x no position has a match


def _parse_refill(x, outcome):
    a = _no_repeat(x + 330, 250, seed=5).copy()
    a[100:105] = _M[:5]
    a[x:x + 5] = _M[:5]
    if outcome == "beaten":
        a[200:207] = _M[1:8]
        a[x + 1:x + 8] = _M[1:8]
    elif outcome == "jump-258":
        a[300:304] = _M[1:5]
        a[x + 1:x + 259] = a[300:558]
    return [a]


def _parse_refill_fact(x, outcome):
    def fact(bufs):
        a, = bufs
        n = len(a)
        assert n < 65536                                              # one block: block positions are the buffer's
        assert (prev_equal(trigrams(a))[REFILL_QUIET:x] == -1).all()  # no match of 3 in front of x: the parse arrives at x idle
        assert longest(a, x, n, 4096)[0] == 5
        after = longest(a, x + 1, n, 4096)[0]
        if outcome == "beaten":
            assert after == 7
        elif outcome == "taken":
            assert after == 4
        else:
            assert after == 258 and x + 1 <= PARSE_CHUNK < x + 259
    return fact


def _refill_outcomes(x):
    """2047 is the last position of the first staged chunk and 2048 the refill: a match held at 2047 is decided on the far
    side; a match of 258 jumps over position 2048 from a start in front of it, or starts on it."""
    return [o for o in REFILL_OUTCOMES if o != "jump-258" or x + 1 <= PARSE_CHUNK]


for _x in REFILL_X:
    for _o in _refill_outcomes(_x):
        _add(f"parse-refill-{_x}-{_o}", functools.partial(_parse_refill, _x, _o), [(8192, 0), (4096, 1000)], _parse_refill_fact(_x, _o),
             f"a match of 5 found at block position {_x}, then {_o}")


# ---- mixtures
def _mixture(i):
    name = f"mixture-{i}"
    r = _rng(name)
    n = int(r.integers(3000, 40001))
    parts, have = [], 0
    while have < n:
        kind = int(r.integers(0, 7))
        m = int(r.integers(200, 6000))
        if kind == 0:
            part = _mixed_bytes(f"{name}-{have}", m)
        elif kind == 1:
            s = int(r.integers(0, 30000))
            part = _no_repeat(5 * 8192 + 3)[s:s + m]
        elif kind == 2:
            part = tc._noise(f"{name}-{have}", m, 250)
            part[m // 2:m // 2 + 3] = MARKER
        elif kind == 3:
            part = tc._zero_heavy(f"{name}-{have}", m, 0.1).copy()
            for length in ZERO_RUNS:
                s = int(r.integers(0, max(1, m - length)))
                part[s:s + length] = 0
        elif kind == 4:
            part = np.tile(tc._zero_heavy(f"{name}-{have}", int(r.integers(3, 600)), 0.6), 12)[:m]
        elif kind == 5:
            part = tc._rows_like(f"{name}-{have}", m)
        else:
            whole = np.concatenate(parts) if parts else tc._noise(name, m)
            s = int(r.integers(0, len(whole)))
            part = whole[s:s + m]
        parts.append(np.asarray(part, dtype=np.uint8))
        have += len(part)
    return [np.concatenate(parts)[:n]]


def _mixture_run(i):
    r = _rng(f"mixture-run-{i}")
    return WINDOWS[int(r.integers(0, len(WINDOWS)))], TILES[int(r.integers(0, len(TILES)))]


def _mixture_fact(bufs):
    a, = bufs
    assert 3000 <= len(a) <= 40000


MIXTURES = [f"mixture-{i}" for i in range(24)]
for _i, _name in enumerate(MIXTURES):
    _add(_name, functools.partial(_mixture, _i), [_mixture_run(_i)], _mixture_fact, "the generators above, glued")

CASE_IDS = list(CASES)


def plan_offsets(bufs):
    """Where the buffers of a call start in the per-position arrays and in the counts' blocks."""
    pos = np.concatenate([[0], np.cumsum([len(b) for b in bufs])])
    blk = np.concatenate([[0], np.cumsum([-(-len(b) // tc.blocksize(len(b))) for b in bufs])])
    return [int(v) for v in pos], [int(v) for v in blk]


# ---- the two sides every test compares with
def cpu_run(exe, tmp, bufs, window, tile):
    """tests/hostlib/png_lodeflate_print.cc's `arrays` mode on the buffers of one call: (sizes, HC, ZC, LD, counts)."""
    import os
    import subprocess
    paths = []
    for i, b in enumerate(bufs):
        paths.append(os.path.join(str(tmp), f"b{i}.bin"))
        b.tofile(paths[-1])
    out = os.path.join(str(tmp), "arrays.bin")
    p = subprocess.run([exe, "arrays", str(window), str(tile), out] + paths, capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    words = np.fromfile(out, dtype="<u4")
    n, blocks = plan_offsets(bufs)
    assert len(words) == 3 * n[-1] + 318 * blocks[-1]
    hc, zc, ld = (words[k * n[-1]:(k + 1) * n[-1]] for k in range(3))
    return [int(v) for v in p.stdout.split()], hc, zc, ld, words[3 * n[-1]:].reshape(blocks[-1], 318)


def ref_library(path):
    """oracle/_ref/libpng_lodeflate_ref.so (tests/hostlib/png_lodeflate_ref.cc): the real LodePNG."""
    import ctypes
    lib = ctypes.CDLL(path)
    lib.ref_png_lo_counts.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint, ctypes.c_void_p, ctypes.c_size_t]
    lib.ref_png_lo_counts.restype = ctypes.c_size_t
    lib.ref_png_lo_zlib_size.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint]
    lib.ref_png_lo_zlib_size.restype = ctypes.c_size_t
    return lib


def ref_run(lib, bufs, window):
    """LodePNG on every buffer of a call: (sizes, counts) laid out as cpu_run's."""
    sizes, counts = [], []
    for b in bufs:
        nblocks = -(-len(b) // tc.blocksize(len(b)))
        c = np.zeros((nblocks, 318), dtype=np.uint32)
        assert lib.ref_png_lo_counts(b.ctypes.data, len(b), window, c.ctypes.data, nblocks) == nblocks
        counts.append(c)
        sizes.append(int(lib.ref_png_lo_zlib_size(b.ctypes.data, len(b), window)))
    return sizes, np.concatenate(counts)


def differences(what, got, want, bufs, tile):
    """The first five words in which two per-position arrays differ: (buffer, position, tile, got, want) in hex."""
    n, _ = plan_offsets(bufs)
    out = []
    for g in np.flatnonzero(got != want)[:5]:
        b = int(np.searchsorted(n, g, side="right")) - 1
        p = int(g) - n[b]
        out.append(f"{what} buffer {b} position {p} tile {p // (tile or DEVICE_TILE)}: {int(got[g]):#010x} != {int(want[g]):#010x}")
    return out
