"""The cases of tests/test_cpu_png_brute_sizes.py and tests/test_gpu_png_brute_sizes.py: small images whose row LENGTHS put
k_png_brute (zopfli_amd/csrc/device/zmx_png_brute.h) on each of its paths — the dynamic LDS and the global scratch on either
side of 16839 bytes, the raised LDS limit on either side of 7281, rows around and beyond every window, chunks of 1024
positions that end one short of, at and one beyond the row's end, rows of one to three bytes — at windows from 1 to 32768.
Every one of an image's 5 * height jobs (row, filter type) is compared in bytes AND bits, with no tolerance.

A case names its row length, the bytes per pixel, the window and a kind per row.  Filter type 0 prices a row's bytes as
they are, so a designed row reaches the deflate stage exactly as written; the types 1 to 4 of the same rows come along.
Every kind has a `fact`: what the real LodePNG's counters (tests/hostlib/png_brute_ref.cc) must show on that row under type
0 for the row to do its job — a match of 258, an offset of window - 1, no match at all on noise, and so on."""
import ctypes
import functools
import os
import subprocess
import zlib

import numpy as np

import png_lodeflate_seam_cases as sc

CHUNK = 1024                 # k_png_brute builds its links 1024 positions at a time
LDS_LAST = 16839             # the longest row whose per-position arrays fit the dynamic LDS (pngb_row_bytes = 148 KiB)
LDS_DEFAULT_LAST = 7281      # the longest row that fits 64 KiB of it, the limit a kernel has before it is raised
FORCE_SCRATCH_MAX = 5000     # every case of rows up to this length runs once more with the arrays in the global scratch
R_MATCHES, R_MAXOFF, R_N258, R_N3, R_FIRST, R_LONGEST = range(6)      # ref_png_brute_sizes' reach counters
KINDS = ("random", "zero-heavy", "zero-runs", "periodic", "hash0", "far3", "flat", "gradient")    # the model tool's eight
FAR = 5000                   # far3's distance: above 4096, where LodePNG makes a literal of a match of 3


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def row_bytes(n):
    """pngb_row_bytes: the per-position arrays of a row of n bytes."""
    return ((n + 3) & ~3) + 8 * n


assert row_bytes(LDS_LAST) == 148 * 1024 < row_bytes(LDS_LAST + 1)
assert row_bytes(LDS_DEFAULT_LAST) <= 64 * 1024 < row_bytes(LDS_DEFAULT_LAST + 1)


# ---- rows
def _noise(name, n):
    """Bytes in which no three occur twice (no LodePNG hash does, and none is 0), for rows of up to 40000 bytes."""
    assert n <= 40000, n
    s = int(_rng(name).integers(0, 40960 - n))
    return sc._no_repeat(5 * 8192 + 3)[s:s + n].copy()


def _plain_noise(name, n):
    return _rng(name).integers(0, 256, n).astype(np.uint8)


def _zero_heavy(name, n):
    r = _rng(name)
    return np.where(r.integers(0, 8, n) == 0, r.integers(0, 256, n), 0).astype(np.uint8)


def _zero_runs(name, n):
    r = _rng(name)
    a = np.zeros(n, dtype=np.uint8)
    i = int(r.integers(0, 600))
    while i < n:
        a[i] = r.integers(1, 256)
        i += 1 + int(r.integers(0, 600))
    return a


def _periodic(name, n):
    r = _rng(name)
    per = 1 + int(r.integers(0, 40))
    a = ((np.arange(n) % per) * 37 & 255).astype(np.uint8)
    a[int(r.integers(0, n))] ^= 1
    return a


def _hash0(name, n):
    return np.tile(np.array([0x10, 0x01, 0x00], dtype=np.uint8), n // 3 + 1)[:n].copy()


def far3_starts(n):
    return range(0, max(0, n - FAR - 4), 997)


def _far3(name, n):
    """Noise with the three bytes at i again at i + 5000 (every 997 positions), the fourth byte made to differ."""
    a = _noise(name, n)
    for i in far3_starts(n):
        a[i + FAR:i + FAR + 3] = a[i:i + 3]
        if a[i + FAR + 3] == a[i + 3]:
            a[i + FAR + 3] ^= 0x80
    return a


def _flat(name, n):
    r = _rng(name)
    return np.where(r.integers(0, 50, n) == 0, r.integers(0, 256, n), 17).astype(np.uint8)


def _flat_rare(name, n):
    """flat with a change in 4000 bytes instead of 50, for the rows beyond 32768 bytes.  A search that starts less than
    nicematch bytes in front of a change finds no match of 128 and walks its whole chain, 32768 links at zopflipng's
    window, out of the scratch in global memory: measured on an MI355X, k_png_brute takes 10 s for one row of 65537 bytes
    of `flat` and 6 s with a change in 400 bytes, whatever the image's height (the jobs run side by side), and LodePNG
    itself 1.4 s per filter type.  The walks over the window's wrap are the same with 16 changes as with 1300."""
    r = _rng(name)
    return np.where(r.integers(0, 4000, n) == 0, r.integers(0, 256, n), 17).astype(np.uint8)


def _gradient(name, n):
    r = _rng(name)
    return ((np.arange(n) // 4) * 3 + r.integers(0, 7, n) - 3 & 255).astype(np.uint8)


def _nonzero_noise(name, n):
    a = _noise(name, n)
    a[a == 0] = 0x81
    return a


def _zrun(length):
    def make(name, n):
        a = _nonzero_noise(name, n)
        start = CHUNK - length // 2
        a[start:start + length] = 0
        return a
    return make


def _zero_tail(name, n):
    a = _nonzero_noise(name, n)
    a[max(1, n - 300):] = 0
    return a


def _seam(src):
    """The three bytes at `src` again at 1500: the key's only earlier position is `src`."""
    def make(name, n):
        a = _noise(name, n)
        a[1500:1503] = a[src:src + 3]
        if a[1503] == a[src + 3]:
            a[1503] ^= 0x80
        return a
    return make


def _edge(window):
    """Twenty bytes again window - 1 further on, the farthest LodePNG can reach, and twenty others exactly a window
    further on, where the slot already holds the new position."""
    def make(name, n):
        assert n >= window + 130
        a = _noise(name, n) if n <= 40000 else _plain_noise(name, n)
        a[5 + window - 1:25 + window - 1] = a[5:25]
        a[100 + window:120 + window] = a[100:120]
        return a
    return make


def _lazy_switch(name, n):
    """With b of 99 bytes and d of 50 that occur nowhere else: [x b] at 100, [y b d] at 300 and [x b d] at 600.  At 600 the
    longest match is [x b], 100 bytes; at 601 it is [b d], 149.  With maxlazymatch 64 (windows below 8192) LodePNG emits
    the 100 at once; with 258 it holds it for a byte and emits the 149 instead.  (The row's first match, [b] at 301 against
    101, is 99 bytes long and comes out the same either way.)"""
    stream = sc._no_repeat(5 * 8192 + 3)
    a, b, d = stream[10000:10000 + n].copy(), stream[13000:13099], stream[13200:13250]
    assert n <= 2900
    a[101:200] = b
    a[301:400], a[400:450] = b, d
    a[600], a[601:700], a[700:750] = a[100], b, d
    assert a[300] != a[100] and a[200] != d[0] and a[450] != a[750]
    return a


MAKERS = {
    "random": _noise, "zero-heavy": _zero_heavy, "zero-runs": _zero_runs, "periodic": _periodic, "hash0": _hash0, "far3": _far3,
    "flat": _flat, "flat-rare": _flat_rare, "gradient": _gradient,
    "zeros": lambda name, n: np.zeros(n, dtype=np.uint8),
    "byte-85": lambda name, n: np.full(n, 85, dtype=np.uint8),
    "zero-tail": _zero_tail, "seam-last-lane": _seam(CHUNK - 1), "seam-lane-0": _seam(CHUNK), "lazy-switch": _lazy_switch,
    "zrun-257": _zrun(257), "zrun-258": _zrun(258), "zrun-259": _zrun(259), "zrun-600": _zrun(600),
    "tiny-noise": _plain_noise,
    "tiny-same": None,       # the row above, again
    "tiny-next": None,       # the row above plus one
}


# ---- what LodePNG's counters must show on a row under filter type 0
def _longest_zero_run(a):
    z = np.flatnonzero(np.concatenate([[1], a, [1]]))
    return int(np.diff(z).max()) - 1


def row_fact(kind, a, r, window):
    n = len(a)
    if window < 8:                                   # maxchainlength = window / 8 = 0: LodePNG never looks
        assert r[R_MATCHES] == 0, (kind, r)
        return
    if r[R_MATCHES]:
        assert 1 <= r[R_MAXOFF] <= window - 1, (kind, r)
    if kind in ("random", "tiny-noise"):
        assert r[R_MATCHES] == 0, (kind, r)
    elif kind == "flat-rare":
        assert r[R_N258] >= 10 and r[R_MATCHES] >= 100, (kind, r)
    elif kind in ("zero-heavy", "flat"):
        assert n < 300 or r[R_MATCHES] >= (10 if kind == "zero-heavy" and window >= 64 else 1), (kind, r)
    elif kind == "zero-runs":
        assert (r[R_N258] >= 1) == (_longest_zero_run(a) >= 259), (kind, r)
    elif kind in ("periodic", "hash0"):
        if n >= (600 if kind == "periodic" else 300) and window >= 64:
            assert r[R_N258] >= 1 and r[R_LONGEST] == 258, (kind, r)
    elif kind == "far3":
        starts = far3_starts(n)
        assert n <= 2 * FAR or len(starts) >= 3
        if window >= 8192:
            assert all((a[i:i + 3] == a[i + FAR:i + FAR + 3]).all() and a[i + 3] != a[i + FAR + 3] for i in starts)
        assert r[R_MATCHES] == 0, (kind, r)          # in reach at 8192 and more, and still literals: the offset > 4096 rule
    elif kind in ("zeros", "byte-85"):
        if n >= 4:
            assert r[R_MAXOFF] == 1 and r[R_N258] == (n - 1) // 258, (kind, r)
        else:
            assert r[R_MATCHES] == 0, (kind, r)
    elif kind == "zero-tail":
        assert r[R_MAXOFF] == 1 and r[R_N258] == 1 and a[-1] == 0 and a[n - 301] != 0, (kind, r)
    elif kind == "seam-last-lane":
        assert (r[R_MATCHES], r[R_MAXOFF], r[R_FIRST]) == (1, 1500 - (CHUNK - 1), 3) and window > 477, (kind, r)
    elif kind == "seam-lane-0":
        assert (r[R_MATCHES], r[R_MAXOFF], r[R_FIRST]) == (1, 1500 - CHUNK, 3) and window > 476, (kind, r)
    elif kind.startswith("zrun-"):
        length = int(kind[5:])
        start = CHUNK - length // 2
        assert sc.exact_zero_run(a, start, length) and start < CHUNK < start + length
        assert r[R_MAXOFF] == 1 and r[R_N258] == (length - 1) // 258 and r[R_LONGEST] == min(258, length - 1), (kind, r)
    elif kind == "edge":
        assert r[R_MAXOFF] == window - 1 and r[R_LONGEST] >= 20, (kind, r)
    elif kind == "lazy-switch":
        assert r[R_FIRST] == 99 and r[R_LONGEST] == (149 if window >= 8192 else 100), (kind, r)
    else:
        assert kind in ("gradient", "tiny-same", "tiny-next"), kind


class Case:
    def __init__(self, name, linebytes, bytewidth, window, kinds, what, grids=(0,), model=True):
        assert linebytes % bytewidth == 0 and bytewidth in (1, 2, 3, 4, 6, 8), (name, linebytes, bytewidth)
        self.name, self.linebytes, self.bytewidth, self.window = name, linebytes, bytewidth, window
        self.kinds, self.what, self.model = tuple(kinds), what, model
        self.height = len(self.kinds)
        # (force_scratch, max_workgroups) of every run on the device
        self.knobs = [(0, g) for g in grids]
        if linebytes <= FORCE_SCRATCH_MAX:
            self.knobs += [(1, 0)]

    @functools.lru_cache(maxsize=None)
    def image(self):
        """[height][linebytes] uint8, read-only."""
        rows = []
        for y, kind in enumerate(self.kinds):
            seed = f"{self.name}/{y}/{kind}"
            if kind == "tiny-same":
                rows.append(rows[-1].copy())
            elif kind == "tiny-next":
                rows.append(rows[-1] + np.uint8(1))
            elif kind == "edge":
                rows.append(_edge(self.window)(seed, self.linebytes))
            else:
                rows.append(MAKERS[kind](seed, self.linebytes))
        img = np.ascontiguousarray(np.stack(rows), dtype=np.uint8)
        assert img.shape == (self.height, self.linebytes)
        img.setflags(write=False)
        return img

    def check(self, reach):
        """The case reaches what it is there for: every row's fact, from LodePNG's counters under filter type 0."""
        img = self.image()
        for y, kind in enumerate(self.kinds):
            row_fact(kind, img[y], [int(v) for v in reach[y, 0]], self.window)
        if self.window < 8:
            assert not reach[:, :, R_MATCHES].any()
        assert (reach[:, :, R_MAXOFF] <= max(0, self.window - 1)).all()


CASES = {}


def _add(*args, **kwargs):
    c = Case(*args, **kwargs)
    assert c.name not in CASES
    CASES[c.name] = c


def _bw(n, prefer=(4, 3, 2, 1)):
    return next(b for b in prefer if n % b == 0)


# ---- the LDS boundary: 16839 bytes is the last row in the dynamic LDS, 16840 the first on the global scratch
for _n in (LDS_LAST, LDS_LAST + 1):
    for _w in (2048, 32768):
        _add(f"lds-edge-{_n}-w{_w}", _n, _bw(_n), _w, ("far3", "zero-runs"), "the last row in the LDS / the first on the scratch")
# ---- the raised LDS limit: 7281 bytes fit 64 KiB, 7282 need hipFuncSetAttribute
for _n in (LDS_DEFAULT_LAST, LDS_DEFAULT_LAST + 1):
    for _w in (2048, 32768):
        _add(f"lds-limit-{_n}-w{_w}", _n, _bw(_n), _w, ("gradient", "zero-heavy"), "64 KiB of dynamic LDS, and the first row beyond")
# ---- rows beyond the window at 32768: the slots wrap, the "keep" walk takes more than one step
# (`flat` rows of these lengths cost the kernel and LodePNG seconds each: flat-rare, see there.  A row of zero runs right
# under a flat or periodic one is such a row under the Up filter — 4 s to 7 s a case —, so a row of noise stands above it.)
for _n in (32767, 32768, 32769):
    _add(f"beyond-w32768-{_n}", _n, _bw(_n), 32768, ("flat-rare", "periodic", "random", "zero-runs"), "a row one short of, at and one beyond zopflipng's window",
         model=False)
_add("beyond-w32768-65537-a", 65537, 1, 32768, ("flat-rare", "periodic"), "two wraps of zopflipng's window", model=False)
_add("beyond-w32768-65537-b", 65537, 1, 32768, ("zero-runs", "edge"), "two wraps of zopflipng's window; a match at offset 32767", model=False)
# ---- the same offsets around the other windows
for _w in (256, 2048, 8192):
    for _n in (_w - 1, _w, _w + 1, 2 * _w + 1):
        _kinds = ["flat", "zero-runs", "periodic"] + (["edge"] if _n >= _w + 130 else []) + (["far3"] if _n > 2 * FAR else [])
        _add(f"beyond-w{_w}-{_n}", _n, _bw(_n), _w, _kinds, f"a row of W - 1, W, W + 1, 2 W + 1 bytes at window {_w}",
             model=(_w < 8192 or _n == _w + 1))
# ---- the window sweep: every kind at every window; 4096 against 8192 is the maxchain / maxlazy switch, below 8 no search
SWEEP_WINDOWS = (1, 2, 4, 8, 64, 4096, 8192, 16384)
for _w in SWEEP_WINDOWS:
    _add(f"sweep-w{_w}-300", 300, 6, _w, KINDS, f"every kind at window {_w}, pixels of 6 bytes")
    _add(f"sweep-w{_w}-5000", 5000, 8, _w, KINDS, f"every kind at window {_w}, pixels of 8 bytes")
for _w in (4096, 8192):
    _add(f"lazy-switch-w{_w}", 2500, 4, _w, ("lazy-switch", "gradient"), "a match of 100 that maxlazymatch 64 takes and 258 trades for 149")
for _w in (8192, 32768):
    _add(f"far3-w{_w}", 12000, 4, _w, ("far3", "far3"), "matches of 3 at distance 5000: literals by the offset > 4096 rule")
# ---- the chunk seams of step 3
for _n in (1023, 1024, 1025, 2049):
    _add(f"chunk-{_n}", _n, _bw(_n), 32768, ("zero-tail", "random", "zero-heavy", "zero-runs", "periodic", "flat", "gradient", "hash0"),
         "a last chunk of 1023, 1024, 1 and 1 positions; a zero run that ends with the row")
for _w in (512, 32768):
    _add(f"chunk-seam-keys-w{_w}", 2049, 3, _w, ("seam-last-lane", "seam-lane-0", "zrun-257", "zrun-258", "zrun-259", "zrun-600"),
         "a key last seen in the previous chunk's last lane, in its own chunk's lane 0; zero runs over position 1024")
# ---- tails and pixels: the short hash, one-pixel-wide images
TINY = ("tiny-noise", "tiny-same", "zeros", "tiny-noise", "tiny-next", "byte-85", "zeros", "tiny-noise")
for _bwidth in (1, 2, 3, 4, 6, 8):
    _add(f"one-pixel-bw{_bwidth}", _bwidth, _bwidth, 2048, TINY, "linebytes == bytewidth: no left neighbour anywhere")
for _n in (2, 3, 5):
    _add(f"tiny-{_n}", _n, 1, 32768, TINY, "rows no longer than the hash's three bytes, and just longer")
# ---- the persistent job loop: one image, grids of 1, 2 and 3 workgroups and the driver's own
MIXED = ("random", "gradient", "zeros", "random", "byte-85", "gradient", "zero-runs", "flat")
_add("job-loop", 5000, 4, 32768, MIXED, "40 jobs on 1, 2, 3 workgroups: an all-zero row before noise, one repeated byte before a gradient",
     grids=(0, 1, 2, 3))

CASE_IDS = list(CASES)


# ---- the sides every test compares
def ref_library(path):
    """oracle/_ref/libpng_brute_ref.so (tests/hostlib/png_brute_ref.cc): the real LodePNG."""
    lib = ctypes.CDLL(path)
    lib.ref_png_brute_sizes.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.ref_png_brute_sizes.restype = ctypes.c_uint
    lib.ref_png_brute_types.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, ctypes.c_void_p]
    lib.ref_png_brute_types.restype = ctypes.c_uint
    return lib


_REF = {}


def ref_run(lib, case):
    """LodePNG on every job of a case, computed once per process: (bytes [h][5], bits [h][5], reach [h][5][6], filter()'s
    types [h]), read-only."""
    if case.name not in _REF:
        img, h = case.image(), case.height
        bits = np.zeros((h, 5), dtype=np.uint64)
        size = np.zeros((h, 5), dtype=np.uint64)
        reach = np.zeros((h, 5, 6), dtype=np.uint32)
        types = np.full(h, 255, dtype=np.uint8)
        assert lib.ref_png_brute_sizes(img.ctypes.data, case.linebytes, h, case.bytewidth, case.window, bits.ctypes.data, size.ctypes.data,
                                       reach.ctypes.data) == 0
        assert lib.ref_png_brute_types(img.ctypes.data, case.linebytes, h, case.bytewidth, case.window, types.ctypes.data) == 0
        for a in (size, bits, reach, types):
            a.setflags(write=False)
        _REF[case.name] = (size, bits, reach, types)
    return _REF[case.name]


def model_run(exe, tmp, case):
    """tests/hostlib/png_brute_print.cc's `sizes` on a case: (bytes [h][5], bits [h][5])."""
    path = os.path.join(str(tmp), "image.bin")
    case.image().tofile(path)
    p = subprocess.run([exe, "sizes", str(case.window), str(case.linebytes), str(case.height), str(case.bytewidth), path],
                       capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    v = np.array(p.stdout.split(), dtype=np.uint64).reshape(case.height, 5, 2)
    return v[:, :, 0], v[:, :, 1]


def first_smallest(sizes):
    """The first smallest of every row's five sizes (lodepng.cpp:5621)."""
    return np.argmin(sizes, axis=1).astype(np.uint8)


def mismatches(got, want):
    """The first ten jobs in which two [h][5] arrays differ: (row, type, got, want)."""
    return [(int(y), int(t), int(got[y, t]), int(want[y, t])) for y, t in np.argwhere(got != want)[:10]]
