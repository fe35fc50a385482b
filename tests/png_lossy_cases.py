"""zopflipng's --lossy_transparent and --lossy_8bit in plain numpy, and the images they are tested on
(tests/test_cpu_png_lossy_cases.py, tests/test_gpu_png_lossy.py).

The model states zopflipng_lib.cc's LossyOptimizeTransparent without its loops, on the image's 8-bit view r, g, b, a
(grey gives r = g = b; a 16-bit sample is its high byte) and its N pixels in raster order, rows back to back:
  key      no pixel has 0 < a < 255
  palette  at most 256 colours, every pixel with a = 0 counting as the one colour 0
  fixed    (key or palette) every pixel with a = 0 gets the RGB of the FIRST such pixel
  carry    (else) a pixel with a = 0 gets the RGB of the last pixel before it, in the whole image, that had a > 0;
           (0, 0, 0) where there was none — np.maximum.accumulate over the opaque pixels' indices
Alpha and the pixels with a > 0 never change.  test_cpu_png_lossy_cases.py holds the model against the all-reference
zopflipng.  A case is (name, width, height, colour type, bit depth); `pixels(case)` gives its (height, linebytes) bytes in
PNG byte order, EXPECT what it has to reach.

The kernels' geometry (zopfli_amd/csrc/device/zmx_png_lossy.h) is named here once; test_cpu_png_lossy_cases.py holds
these names to the header through tests/hostlib/png_lossy_print.cc, so that "a tile edge" in a case is the kernel's."""
import numpy as np

import png_color_cases as cc
from png_encode_cases import CHANNELS

CHUNK_BYTES = 48          # a thread takes a step
THREADS = 256             # a workgroup; a wave is 64 of them
WAVE = 64
MAX_GROUPS = 2048         # of a launch
SCAN_STEP = 256           # tiles k_png_lossy_carry takes a step


def chunk_pixels(ct, depth):
    return CHUNK_BYTES // (CHANNELS[ct] * depth // 8)


def wave_pixels(ct, depth):
    return WAVE * chunk_pixels(ct, depth)


def tile_pixels(ct, depth):
    return THREADS * chunk_pixels(ct, depth)


def sweep_pixels(ct, depth):
    return MAX_GROUPS * tile_pixels(ct, depth)


C, W, T = chunk_pixels(6, 8), wave_pixels(6, 8), tile_pixels(6, 8)   # RGBA8: 12, 768, 3072
SWEEP = sweep_pixels(6, 8)                                           # 6 291 456

MODE_NONE, MODE_FIXED, MODE_CARRY = 0, 1, 2
TRANSPARENT, EIGHT_BIT = 1, 2   # ZMX_PNG_LOSSY_*


# ---- the model
def view8(img, w, h, ct, depth):
    """(h * w, 4) uint8: r, g, b, a of the 8-bit view."""
    ch, sb = CHANNELS[ct], depth // 8
    s = np.asarray(img).reshape(h * w, ch, sb)[:, :, 0]
    full = np.full(h * w, 255, dtype=np.uint8)
    if ct in (0, 4):
        cols = [s[:, 0]] * 3 + [full if ct == 0 else s[:, 1]]
    else:
        cols = [s[:, 0], s[:, 1], s[:, 2], full if ct == 2 else s[:, 3]]
    return np.stack(cols, axis=1)


def lossy_transparent(img, w, h, ct, depth, wrong=None):
    """(info, rewritten image): info as zmx_png_lossy_info, the image (h, linebytes) uint8.  `wrong` names a mistaken
    variant of a rule (test_cpu_png_lossy_cases.py: the cases tell each from the right one)."""
    img = np.asarray(img)
    none = {"mode": MODE_NONE, "partial_alpha": 0, "numcolors": 0, "fill": (0, 0, 0), "first_transparent": None}
    v = view8(img, w, h, ct, depth)
    n = h * w
    a = v[:, 3].astype(np.uint32)
    partial = (a > 0) & (a < 255)
    if wrong == "partial-includes-0":
        partial = a < 255
    if wrong == "partial-below-254":
        partial = (a > 0) & (a < 254)
    if wrong == "partial-above-1":
        partial = (a > 1) & (a < 255)
    key = not bool(np.any(partial))
    packed = v[:, 0].astype(np.uint32) | (v[:, 1].astype(np.uint32) << 8) | (v[:, 2].astype(np.uint32) << 16) | (a << 24)
    if wrong != "transparent-by-rgb":
        packed = np.where(a == 0, 0, packed)
    numcolors = min(len(np.unique(packed)), 257)
    palette = numcolors <= {"threshold-255": 255, "threshold-257": 257}.get(wrong, 256)
    info = dict(none, partial_alpha=int(bool(np.any((a > 0) & (a < 255)))), numcolors=numcolors)
    clear = np.nonzero(a == 0)[0]
    if ct in (0, 2) or len(clear) == 0:
        return info, img.copy()
    first = int(clear[-1] if wrong == "last-transparent" else clear[0])
    fixed = key or palette
    if wrong == "carry-despite-palette":
        fixed = key
    if wrong == "fixed-always":
        fixed = True
    rgb = v[:, :3].copy()
    if fixed:
        rgb[clear] = v[first, :3]
        info.update(mode=MODE_FIXED, fill=tuple(int(x) for x in v[first, :3]), first_transparent=int(clear[0]))
    else:
        at = np.arange(n)
        idx = np.where(a > 0, at, -1)
        if wrong == "carry-resets-at-row":
            last = np.maximum.accumulate(idx.reshape(h, w), axis=1).reshape(n)
        elif wrong == "carry-resets-at-tile":
            t = tile_pixels(ct, depth)
            pad = np.full((-n) % t, -1)
            last = np.maximum.accumulate(np.concatenate([idx, pad]).reshape(-1, t), axis=1).reshape(-1)[:n]
        else:
            last = np.maximum.accumulate(idx)
        carried = np.where((last >= 0)[:, None], v[np.maximum(last, 0), :3], 0).astype(np.uint8)
        rgb[clear] = carried[clear]
        info.update(mode=MODE_CARRY, first_transparent=int(clear[0]))
    ch, sb = CHANNELS[ct], depth // 8
    out = img.copy().reshape(n, ch, sb)
    for k in range(ch - 1):
        out[:, k, 0] = rgb[:, k]
    if wrong == "alpha-touched":
        out[clear, ch - 1, 0] = 1
    if wrong == "opaque-touched" and len(clear) < n:
        out[np.nonzero(a > 0)[0][-1], 0, 0] ^= 1
    return info, out.reshape(h, -1)


def to_8bit(img, w, h, ct, depth, wrong=None):
    """--lossy_8bit without --keepcolortype: the high byte of every sample."""
    if depth == 8:
        return np.asarray(img).copy()
    return np.ascontiguousarray(np.asarray(img).reshape(h, w * CHANNELS[ct], 2)[:, :, 1 if wrong == "low-byte" else 0])


WRONG = ["carry-resets-at-row", "carry-resets-at-tile", "last-transparent", "partial-includes-0", "partial-below-254", "partial-above-1",
         "transparent-by-rgb", "threshold-255", "threshold-257", "carry-despite-palette", "fixed-always", "alpha-touched", "opaque-touched"]


def prepared(case, flags, optimize):
    """What the entries encode: (image, depth) after rule 6 — _8BIT counts for the optimize entry and a 16-bit image
    only, _TRANSPARENT for an image that is 8-bit by then."""
    name, w, h, ct, depth = case
    img = pixels(case)
    if optimize and (flags & EIGHT_BIT) and depth == 16:
        img, depth = to_8bit(img, w, h, ct, depth), 8
    if (flags & TRANSPARENT) and depth == 8:
        img = lossy_transparent(img, w, h, ct, depth)[1]
    return np.ascontiguousarray(img), depth


def reduced(img, w, h, ct, depth):
    """png_color_cases' model on an image: (rgba, stats, mode)."""
    rgba = cc.expand(img, w, h, ct, depth)
    st = cc.stats(rgba, depth)
    return rgba, st, cc.choose(st, w * h)


# ---- the images: (n, 4) r, g, b, a of the 8-bit view first
def _rng(name):
    return np.random.default_rng(sum(name.encode()) * 7919 + len(name))


def _busy(rng, n, ct, alpha_low=1, alpha_high=255):
    """n pixels, none transparent, far more than 256 colours where n allows; partial alpha unless alpha_low is 255."""
    v = rng.integers(0, 256, size=(n, 4)).astype(np.uint8)
    v[:, 3] = rng.integers(alpha_low, alpha_high + 1, size=n)
    if ct == 4:
        v[:, 1] = v[:, 2] = v[:, 0]
    return v


def _garbage(rng, v, where):
    """The pixels `where` made transparent, each with an RGB of its own kind."""
    where = np.asarray(where)
    v[where, :3] = rng.integers(0, 256, size=(len(where), 3))
    v[where, 3] = 0
    return v


def _few(rng, n, k, alpha=255):
    """n pixels of k opaque colours (alpha: every one's), every colour at least once where n allows."""
    seen = set()
    while len(seen) < k:
        seen.add(tuple(int(x) for x in rng.integers(0, 256, size=3)))
    colors = np.array(sorted(seen), dtype=np.uint8)[rng.permutation(k)]
    idx = rng.integers(0, k, size=n)
    idx[:min(n, k)] = np.arange(min(n, k))
    return np.concatenate([colors[idx], np.full((n, 1), alpha, dtype=np.uint8)], axis=1)


def _runs(n, *spans):
    return np.unique(np.concatenate([np.arange(a, min(b, n)) for a, b in spans]))


def _make(name, w, h, ct, depth):
    rng = _rng(name)
    n = w * h
    c, wv, t = chunk_pixels(ct, depth), wave_pixels(ct, depth), tile_pixels(ct, depth)
    if name == "one-transparent":
        return np.array([[5, 6, 7, 0]], dtype=np.uint8)
    if name == "one-opaque":
        return np.array([[5, 6, 7, 255]], dtype=np.uint8)
    if name == "no-transparent":
        return _busy(rng, n, ct)
    if name == "all-transparent":
        return _garbage(rng, _busy(rng, n, ct), np.arange(n))
    if name == "carry-leading":
        return _garbage(rng, _busy(rng, n, ct), np.arange(5))
    if name.startswith("first-at-"):
        # key mode (no partial alpha, many colours): the fill is the FIRST transparent pixel's, a later one has another RGB
        at = {"0": 0, "last": n - 1}.get(name[9:])
        if at is None:
            edge, off = name[9:].rsplit("-", 1) if name[9:].count("-") else (name[9:], "0")
            at = {"chunk": c, "wave": wv, "tile": t}[edge] + {"m1": -1, "0": 0, "p1": 1}[off]
        v = _busy(rng, n, ct, 255)
        later = [] if at == n - 1 else [n - 2] if at < n - 2 else []
        v = _garbage(rng, v, [at] + later + ([at + 1] if at + 1 < n - 2 else []))
        v[at, :3] = (9, 9, 9) if ct == 4 else (9, 8, 7)
        return v
    runs = {
        "run-row-end": [(w - 7, w + 8), (5 * w - 1, 5 * w + 1)],
        "run-chunk": [(c - 4, c + 4), (5 * c - 1, 5 * c + 1)],
        "run-wave": [(wv - 8, wv + 7)],
        "run-tile": [(t - 12, t + 13)],
        "run-tiles": [(t - 72, 3 * t + 10), (4 * t, 4 * t + 1)],
        "run-scan-step": [((SCAN_STEP - 2) * t + 5, (SCAN_STEP + 2) * t + 7), (3 * t - 1, 3 * t + 1)],
        "run-sweep": [(sweep_pixels(ct, depth) - 2 * t - 9, sweep_pixels(ct, depth) + t + 9), (7 * t - 3, 9 * t + 3)],
        "tile-end-opaque": [(t, t + 3)],                  # the tile's last pixel opaque, the next tile's first transparent
        "tile-end-transparent": [(t - 3, t)],             # and the reverse
        "ga-carry": [(w - 3, w + 3), (c - 2, c + 2), (wv - 2, wv + 2), (t - 2, t + 2), (0, 2)],
        "w1-column": [(3, 9), (c - 1, c + 1)],
        "w7-ga": [(5, 9), (c - 1, c + 1)],
        "w37": [(30, 45), (c - 1, c + 1)],
        "stays-rgba": [(0, 3), (40, 95), (300, 420)],
    }
    if name in runs:
        return _garbage(rng, _busy(rng, n, ct), _runs(n, *runs[name]))
    if name in ("alpha-1-last", "alpha-254-last"):
        # without the last pixel: key mode
        v = _garbage(rng, _busy(rng, n, ct, 255), _runs(n, (10, 30), (t - 5, t + 5)))
        v[n - 1, 3] = 1 if name == "alpha-1-last" else 254
        return v
    if name in ("pal-255-and-transparent", "pal-256-and-transparent", "zero-beside"):
        k = 256 if name == "pal-256-and-transparent" else 255
        v = _few(rng, n, k)
        v[(v[:, :3] == v[0, :3]).all(axis=1), 3] = 128          # (one of the k colours has a partial alpha)
        spare = rng.permutation(np.arange(k + 1, n))[:n // 4]
        v = _garbage(rng, v, spare)
        if name == "zero-beside":
            v[spare[:3], :3] = 0
        # (the k colours are all still there: the first k pixels were not touched)
        return v
    if name in ("opaque-256", "opaque-257"):
        return _few(rng, n, int(name[7:]))
    if name == "many-transparent-rgbs":
        v = _few(rng, n, 40, alpha=200)
        return _garbage(rng, v, rng.permutation(np.arange(40, n))[:n // 2])
    if name == "257th-last-tile":
        v = _few(rng, n, 255, alpha=77)
        v = _garbage(rng, v, _runs(n, (300, 340), (t - 4, t + 4), (2 * t + 50, 2 * t + 90)))
        v[2 * t + 20] = (1, 2, 3, 78)     # 255 + the transparent one + this: 257
        return v
    if name == "ga-key":
        v = _garbage(rng, _busy(rng, n, ct, 255), _runs(n, (w - 2, w + 2), (c, c + 1)))
        return v
    if name in ("rgba16-hi", "ga16-hi"):
        return _garbage(rng, _busy(rng, n, ct), _runs(n, (w - 3, w + 4), (c - 1, c + 1), (0, 1)))
    if name == "fake16-key":
        return _garbage(rng, _busy(rng, n, ct, 255), _runs(n, (20, 26)))
    if name == "buys-key":
        v = _busy(rng, n, ct, 255)
        v[v[:, 0] == 1, 0] = 2              # (no opaque pixel has the key's RGB)
        v = _garbage(rng, v, _runs(n, (33, 60), (200, 203)))
        v[33, :3] = (1, 2, 3)
        return v
    if name == "buys-palette":
        v = _few(rng, n, 40, alpha=200)
        return _garbage(rng, v, rng.permutation(np.arange(40, n))[:n // 3])
    if name == "buys-grey-key":
        v = _busy(rng, n, ct, 255)
        v[v[:, 0] == 7] = (8, 8, 8, 255)
        v = _garbage(rng, v, _runs(n, (10, 40)))
        v[10, :3] = 7
        return v
    if name in ("retry-wins", "retry-loses"):
        if name == "retry-wins":
            k = (np.arange(n) // 2).astype(np.uint32)
            v = np.stack([40 + 3 * k, 90 + 2 * k, 200 - k, np.full_like(k, 255)], axis=1).astype(np.uint8)
            return _garbage(rng, v, np.arange(n - 9, n - 2))
        seen = set()
        while len(seen) < 100:
            seen.add(tuple(int(x) for x in rng.integers(1, 255, size=4)))
        colors = np.array(sorted(seen), dtype=np.uint8)
        idx = rng.integers(0, 100, size=n)
        idx[rng.permutation(n)[:100]] = np.arange(100)
        return _garbage(rng, colors[idx], rng.permutation(n)[:40])
    raise KeyError(name)


_N_FIRST = (2 * T + 139) // 61 * 61
CASES = [
    ("one-transparent", 1, 1, 6, 8), ("one-opaque", 1, 1, 6, 8), ("no-transparent", 20, 13, 6, 8), ("all-transparent", 17, 9, 6, 8),
    ("carry-leading", 40, 30, 6, 8),
] + [(f"first-at-{p}", 61, _N_FIRST // 61, 6, 8) for p in ("0", "last", "chunk-m1", "chunk", "chunk-p1", "wave-m1", "wave", "wave-p1",
                                                         "tile-m1", "tile", "tile-p1")] + [
    ("run-row-end", 37, 19, 6, 8), ("run-chunk", 33, 17, 6, 8), ("run-wave", 41, 29, 6, 8), ("run-tile", 67, 71, 6, 8),
    ("run-tiles", 101, 131, 6, 8), ("tile-end-opaque", 67, 71, 6, 8), ("tile-end-transparent", 67, 71, 6, 8),
    ("run-scan-step", 1024, 780, 6, 8), ("run-sweep", 2048, 3080, 6, 8),
    ("alpha-1-last", 67, 71, 6, 8), ("alpha-254-last", 67, 71, 6, 8),
    ("pal-255-and-transparent", 45, 31, 6, 8), ("pal-256-and-transparent", 45, 31, 6, 8), ("opaque-256", 40, 30, 6, 8),
    ("opaque-257", 40, 30, 6, 8), ("many-transparent-rgbs", 97, 83, 6, 8), ("zero-beside", 45, 31, 6, 8),
    ("257th-last-tile", 83, 101, 6, 8),
    ("ga-carry", 89, 83, 4, 8), ("ga-key", 37, 23, 4, 8), ("w1-column", 1, 311, 6, 8), ("w7-ga", 7, 61, 4, 8), ("w37", 37, 11, 6, 8),
    ("rgba16-hi", 29, 17, 6, 16), ("ga16-hi", 31, 19, 4, 16), ("fake16-key", 23, 17, 6, 16),
    ("buys-key", 30, 20, 6, 8), ("buys-palette", 64, 48, 6, 8), ("buys-grey-key", 25, 16, 4, 8), ("retry-wins", 10, 8, 6, 8),
    ("retry-loses", 16, 16, 6, 8), ("stays-rgba", 32, 24, 6, 8), ("idempotent", 32, 24, 6, 8),
]
IDS = [c[0] for c in CASES]
LARGE = {"run-scan-step", "run-sweep"}          # the step alone: the library deflates nothing for them
SWEEP_CASES = {"run-sweep"}                     # beyond one sweep of a full launch: a test of its own (25 MB)
ENTRY_CASES = ["buys-key", "buys-palette", "buys-grey-key", "retry-wins", "retry-loses", "stays-rgba", "idempotent", "rgba16-hi", "ga16-hi",
               "fake16-key", "no-transparent"]
_PIXELS = {}


def case(name):
    return CASES[IDS.index(name)]


def pixels(case):
    """(height, linebytes) uint8, PNG byte order; made once and never changed."""
    name, w, h, ct, depth = case
    if name not in _PIXELS:
        if name == "idempotent":
            img = lossy_transparent(pixels(CASES[IDS.index("stays-rgba")]), w, h, ct, depth)[1]
        else:
            v = _make(name, w, h, ct, depth)
            assert v.shape == (w * h, 4) and v.dtype == np.uint8, name
            s = {4: v[:, [0, 3]], 6: v}[ct]
            if depth == 16:
                # the low bytes differ from the high ones and from each other (fake16-*: they are the high ones again)
                low = s if name.startswith("fake16") else (s.astype(np.uint32) * 7 + np.arange(s.size).reshape(s.shape) + 1).astype(np.uint8)
                s = np.stack([s, low], axis=2)
            img = np.ascontiguousarray(s).reshape(h, -1)
        img.setflags(write=False)
        _PIXELS[name] = img
    return _PIXELS[name]


_MODEL = {}


def model(case):
    """(info, rewritten image) of a case, computed once."""
    name, w, h, ct, depth = case
    if name not in _MODEL:
        info, out = lossy_transparent(pixels(case), w, h, ct, depth)
        out.setflags(write=False)
        _MODEL[name] = (info, out)
    return _MODEL[name]


def mode_tuple(mode):
    return (mode["colortype"], mode["bitdepth"], 0 if mode["palette"] is None else len(mode["palette"]), mode["key"])


# What every case has to reach: (mode, key, palette, first transparent index: None without one) of the step.  A case that
# ends elsewhere no longer tests its edge.
_F = _N_FIRST
EXPECT = {
    "one-transparent": (1, True, True, 0), "one-opaque": (0, True, True, None), "no-transparent": (0, False, False, None),
    "all-transparent": (1, True, True, 0), "carry-leading": (2, False, False, 0),
    "first-at-0": (1, True, False, 0), "first-at-last": (1, True, False, _F - 1),
    "first-at-chunk-m1": (1, True, False, C - 1), "first-at-chunk": (1, True, False, C), "first-at-chunk-p1": (1, True, False, C + 1),
    "first-at-wave-m1": (1, True, False, W - 1), "first-at-wave": (1, True, False, W), "first-at-wave-p1": (1, True, False, W + 1),
    "first-at-tile-m1": (1, True, False, T - 1), "first-at-tile": (1, True, False, T), "first-at-tile-p1": (1, True, False, T + 1),
    "run-row-end": (2, False, False, 30), "run-chunk": (2, False, False, C - 4), "run-wave": (2, False, False, W - 8),
    "run-tile": (2, False, False, T - 12), "run-tiles": (2, False, False, T - 72), "tile-end-opaque": (2, False, False, T),
    "tile-end-transparent": (2, False, False, T - 3), "run-scan-step": (2, False, False, 3 * T - 1), "run-sweep": (2, False, False, 7 * T - 3),
    "alpha-1-last": (2, False, False, 10), "alpha-254-last": (2, False, False, 10),
    "pal-255-and-transparent": (1, False, True, 259), "pal-256-and-transparent": (2, False, False, 257),
    "opaque-256": (0, True, True, None), "opaque-257": (0, True, False, None), "many-transparent-rgbs": (1, False, True, 40),
    "zero-beside": (1, False, True, 256), "257th-last-tile": (2, False, False, 300),
    "ga-carry": (2, False, False, 0), "ga-key": (1, True, True, 24), "w1-column": (2, False, False, 3), "w7-ga": (2, False, False, 5),
    "w37": (2, False, False, 11), "rgba16-hi": (2, False, False, 0), "ga16-hi": (2, False, False, 0), "fake16-key": (1, True, False, 20),
    "buys-key": (1, True, False, 33), "buys-palette": (1, False, True, 40), "buys-grey-key": (1, True, True, 10),
    "retry-wins": (1, True, True, 71), "retry-loses": (1, False, True, 10), "stays-rgba": (2, False, False, 0),
    "idempotent": (2, False, False, 0),
}

# For the entries' cases: the colour mode (colour type, bit depth, palette size, key) of zmx_png_optimize_device_lossy's first
# file under lossy = 0, _TRANSPARENT, _8BIT, both.  tRNS appears only with the flag, a palette only with the flag.
_RGBA, _GA = (6, 8, 0, None), (4, 8, 0, None)
OPTIMIZE_EXPECT = {
    "buys-key": [_RGBA, (2, 8, 0, (1, 2, 3)), _RGBA, (2, 8, 0, (1, 2, 3))],
    "buys-palette": [_RGBA, (3, 8, 41, None), _RGBA, (3, 8, 41, None)],
    "buys-grey-key": [_GA, (0, 8, 0, (7, 7, 7)), _GA, (0, 8, 0, (7, 7, 7))],
    "retry-wins": [_RGBA, (3, 8, 38, None), _RGBA, (3, 8, 38, None)],
    "retry-loses": [_RGBA, (3, 8, 97, None), _RGBA, (3, 8, 97, None)],
    "stays-rgba": [_RGBA] * 4,
    "idempotent": [_RGBA] * 4,
    "rgba16-hi": [(6, 16, 0, None), (6, 16, 0, None), _RGBA, _RGBA],
    "ga16-hi": [(4, 16, 0, None), (4, 16, 0, None), _GA, _GA],
    "fake16-key": [_RGBA, _RGBA, _RGBA, (2, 8, 0, (45, 14, 218))],
    "no-transparent": [_RGBA] * 4,
}
# the second try under strategy 0 and 2 iterations with _TRANSPARENT: whether it replaced the palette file
RETRY_EXPECT = {"retry-wins": True, "retry-loses": False}
