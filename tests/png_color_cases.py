"""Colour-type reduction in plain numpy, and the images it is tested on (tests/test_cpu_png_color_cases.py,
tests/test_gpu_png_color.py, tests/test_gpu_png_optimize.py).

The model states LodePNG's lodepng_compute_color_stats, auto_choose_color and lodepng_convert, and zopflipng's second try
at small palette files, without their loops: every rule on the RGBA expansion of the image (grey gives r = g = b, no
alpha channel gives the maximum), colours in the order of their first appearance.  test_cpu_png_color_cases.py holds it
against the all-reference zopflipng.  A case is (name, width, height, colour type, bit depth); `pixels(case)` gives its
(height, linebytes) bytes in PNG byte order, EXPECT what it has to reach."""
import struct

import numpy as np

from png_encode_cases import CHANNELS, chunk

RETRY_BELOW = 4096


# ---- the model
def expand(img, w, h, ct, depth):
    """(h * w, 4) r, g, b, a at the image's own depth."""
    ch = CHANNELS[ct]
    if depth == 16:
        s = img.reshape(h, w, ch, 2).astype(np.uint32)
        s = (s[..., 0] << 8) | s[..., 1]
    else:
        s = img.reshape(h, w, ch).astype(np.uint32)
    s = s.reshape(h * w, ch)
    full = np.full(h * w, 65535 if depth == 16 else 255, dtype=np.uint32)
    if ct == 0:
        cols = [s[:, 0], s[:, 0], s[:, 0], full]
    elif ct == 2:
        cols = [s[:, 0], s[:, 1], s[:, 2], full]
    elif ct == 4:
        cols = [s[:, 0], s[:, 0], s[:, 0], s[:, 1]]
    else:
        cols = [s[:, 0], s[:, 1], s[:, 2], s[:, 3]]
    return np.stack(cols, axis=1)


def value_bits(v):
    if v in (0, 255):
        return 1
    if v % 17 == 0:
        return 2 if v % 85 == 0 else 4
    return 8


def stats(rgba, depth):
    """LodePNG's colour statistics: colored, key, alpha, numcolors (257: more than 256), bits, key_rgb (16-bit values,
    zeros without a key), palette ((numcolors, 4) bytes in first-appearance order; empty for 0 and 257)."""
    sixteen = depth == 16 and bool(np.any((rgba & 255) != (rgba >> 8)))
    v = rgba if (sixteen or depth == 8) else rgba >> 8
    top = 65535 if sixteen else 255
    r, g, b, a = v[:, 0], v[:, 1], v[:, 2], v[:, 3]
    colored = bool(np.any((r != g) | (r != b)))
    alpha, key, key_rgb = False, False, (0, 0, 0)
    clear = a == 0
    if np.any((a != 0) & (a != top)):
        alpha = True
    elif np.any(clear):
        rgbs = np.unique(v[clear, :3], axis=0)
        if len(rgbs) == 1 and not np.any(~clear & np.all(v[:, :3] == rgbs[0], axis=1)):
            key = True
            key_rgb = tuple(int(x) * (1 if sixteen else 257) for x in rgbs[0])
        else:
            alpha = True
    out = {"colored": colored, "key": key, "alpha": alpha, "key_rgb": key_rgb, "numcolors": 0,
           "palette": np.zeros((0, 4), dtype=np.uint8)}
    if sixteen:
        out["bits"] = 16
        return out
    bits = max(value_bits(int(x)) for x in np.unique(r))
    out["bits"] = 8 if (colored or alpha) else bits
    packed = (r.astype(np.uint64) << 24) | (g.astype(np.uint64) << 16) | (b.astype(np.uint64) << 8) | a.astype(np.uint64)
    _, first = np.unique(packed, return_index=True)
    first = np.sort(first)
    if len(first) > 256:
        out["numcolors"] = 257
    else:
        out["numcolors"] = len(first)
        out["palette"] = v[first].astype(np.uint8)
    return out


def choose(st, numpixels):
    """auto_choose_color: {colortype, bitdepth, palette ((n, 4) or None), key (three values or None)}."""
    alpha, key, bits = st["alpha"], st["key"], st["bits"]
    if key and numpixels <= 16:
        alpha, key, bits = True, False, max(bits, 8)
    gray_ok = not st["colored"]
    if not gray_ok:
        bits = max(bits, 8)
    n = st["numcolors"]
    palettebits = 1 if n <= 2 else 2 if n <= 4 else 4 if n <= 16 else 8
    palette_ok = n <= 256 and bits <= 8 and n != 0
    if numpixels < 2 * n:
        palette_ok = False
    if gray_ok and not alpha and bits <= palettebits:
        palette_ok = False
    if palette_ok:
        return {"colortype": 3, "bitdepth": palettebits, "palette": st["palette"], "key": None}
    ct = (4 if gray_ok else 6) if alpha else (0 if gray_ok else 2)
    mask = (1 << bits) - 1
    return {"colortype": ct, "bitdepth": bits, "palette": None, "key": tuple(x & mask for x in st["key_rgb"]) if key else None}


def retry_mode(st, numpixels):
    """What zopflipng tries as well for a palette file below 4096 bytes."""
    alpha = st["alpha"] or (numpixels <= 16 and st["key"])
    key = tuple(x & 255 for x in st["key_rgb"]) if (st["key"] and not alpha) else None
    return {"colortype": 6 if alpha else 2, "bitdepth": 8, "palette": None, "key": key}


def bpp(mode):
    return (1 if mode["colortype"] == 3 else CHANNELS[mode["colortype"]]) * mode["bitdepth"]


def rowbytes(w, mode):
    return (w * bpp(mode) + 7) // 8


def bytewidth(mode):
    return max(1, bpp(mode) // 8)


def convert(rgba, depth, w, h, mode):
    """(h, rowbytes) bytes of the image in `mode`."""
    ct, d = mode["colortype"], mode["bitdepth"]
    if d == 16:
        assert depth == 16
        v = rgba
    else:
        v = rgba >> 8 if depth == 16 else rgba
    if ct == 3:
        pal = [tuple(int(x) for x in e) for e in mode["palette"]]
        rank = {c: i for i, c in enumerate(pal)}   # (of two equal entries the later one)
        vals = np.array([rank[tuple(int(x) for x in px)] for px in v], dtype=np.uint32)[:, None]
    elif ct == 0:
        vals = v[:, :1] if d >= 8 else v[:, :1] >> (8 - d)
    elif ct == 2:
        vals = v[:, :3]
    elif ct == 4:
        vals = v[:, [0, 3]]
    else:
        vals = v
    vals = vals.reshape(h, w * vals.shape[1])
    if d == 16:
        return np.stack([vals >> 8, vals & 255], axis=2).reshape(h, -1).astype(np.uint8)
    if d == 8:
        return vals.astype(np.uint8)
    bits = ((vals[:, :, None] >> np.arange(d - 1, -1, -1)) & 1).astype(np.uint8).reshape(h, -1)
    return np.packbits(bits, axis=1)


def same_mode(ct, depth, mode):
    return mode["colortype"] == ct and mode["bitdepth"] == depth and mode["key"] is None


# ---- the container
def ihdr(w, h, mode):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, mode["bitdepth"], mode["colortype"], 0, 0, 0))


def color_chunks(mode):
    """PLTE and tRNS as LodePNG writes them."""
    out = b""
    if mode["colortype"] == 3:
        pal = np.asarray(mode["palette"], dtype=np.uint8)
        out += chunk(b"PLTE", pal[:, :3].tobytes())
        notopaque = np.nonzero(pal[:, 3] != 255)[0]
        if len(notopaque):
            out += chunk(b"tRNS", pal[: notopaque[-1] + 1, 3].tobytes())
    elif mode["key"] is not None:
        k = mode["key"]
        out += chunk(b"tRNS", struct.pack(">H", k[0]) if mode["colortype"] == 0 else struct.pack(">HHH", *k))
    return out


def assemble(w, h, mode, zlib_stream):
    """The file zmx_png_optimize_device promises around zopfli's zlib stream of the filtered scanlines (78 DA ...)."""
    assert zlib_stream[:2] == b"\x78\xda"
    return (b"\x89PNG\r\n\x1a\n" + ihdr(w, h, mode) + color_chunks(mode) + chunk(b"IDAT", b"\x78\x01" + zlib_stream[2:]) +
            chunk(b"IEND", b""))


def expected_chunks(mode):
    tags = [b"IHDR"]
    if mode["colortype"] == 3:
        tags.append(b"PLTE")
        if np.any(np.asarray(mode["palette"])[:, 3] != 255):
            tags.append(b"tRNS")
    elif mode["key"] is not None:
        tags.append(b"tRNS")
    return tags + [b"IDAT", b"IEND"]


# ---- the images
def _bytes(samples, depth):
    """(h, w, channels) sample values -> (h, linebytes) uint8 in PNG byte order."""
    h = samples.shape[0]
    if depth == 16:
        return np.ascontiguousarray(samples).astype(">u2").view(np.uint8).reshape(h, -1)
    return samples.astype(np.uint8).reshape(h, -1)


def _as(rgba, ct):
    """(h, w, 4) -> the channels colour type `ct` keeps."""
    return {0: rgba[..., :1], 2: rgba[..., :3], 4: rgba[..., [0, 3]], 6: rgba}[ct]


def _colors(rng, n, alpha=False):
    """n distinct coloured RGBA values, opaque unless `alpha`."""
    seen = set()
    while len(seen) < n:
        c = tuple(int(x) for x in rng.integers(0, 256, size=4))
        if c[0] == c[1] == c[2]:
            continue
        seen.add(c if alpha else c[:3] + (255,))
    return np.array(sorted(seen), dtype=np.uint32)[rng.permutation(n)]


def _tiled(rng, w, h, colors):
    """Every colour at least once, first appearances in the colours' order, then at random."""
    n = len(colors)
    idx = rng.integers(0, n, size=w * h)
    idx[:n] = np.arange(n)
    return colors[idx].reshape(h, w, 4)


def _grey_levels(rng, w, h, bits):
    levels = np.arange(1 << bits, dtype=np.uint32) * (255 // ((1 << bits) - 1)) if bits < 8 else np.arange(256, dtype=np.uint32)
    g = levels[rng.integers(0, len(levels), size=(h, w))]
    if bits < 8 and w * h >= 2:
        g.flat[0], g.flat[-1] = levels[1], levels[-2]   # (a value that needs all the bits: not only 0 and 255)
    elif bits == 8 and w * h >= 1:
        g.flat[0] = 3
    return np.stack([g, g, g, np.full_like(g, 255)], axis=2)


def _make(name, w, h, ct, depth):
    rng = np.random.default_rng(sum(name.encode()) * 7919 + w * 31 + h)
    kind = name.split("-w")[0] if name.startswith("grey") and "-w" in name else name
    if name.startswith("colors-") and name.split("-")[1].isdigit() and len(name.split("-")) == 2:
        return _tiled(rng, w, h, _colors(rng, int(name.split("-")[1])))
    if name == "colors-256-spread":
        colors = _colors(rng, 256)
        n = w * h
        born = np.minimum(np.arange(n) // (n // 256), 255)            # the newest colour a pixel may have
        idx = (rng.integers(0, 1 << 30, size=n) % (born + 1))
        idx[np.arange(256) * (n // 256)] = np.arange(256)
        return colors[idx].reshape(h, w, 4)
    if name == "colors-last-pixel":
        img = _tiled(rng, w, h, _colors(rng, 3)[:2])
        img[-1, -1] = (9, 200, 31, 255)
        return img
    if name == "colors-alpha-only":
        colors = np.array([(10, 20, 30, a) for a in (255, 200, 100, 50)] + [(r, 20, 30, 255) for r in (11, 12)], dtype=np.uint32)
        return _tiled(rng, w, h, colors)
    if name == "colors-00-ff":
        colors = np.array([(0, 0, 0, 0), (255, 255, 255, 255), (255, 0, 0, 255), (255, 255, 255, 0)], dtype=np.uint32)
        return _tiled(rng, w, h, colors)
    if name == "colors-257th-last":
        colors = _colors(rng, 257)
        img = _tiled(rng, w, h, colors[:256])
        img[-1, -1] = colors[256]
        return img
    if name in ("key", "key-opaque-before", "key-opaque-after", "key-two-rgbs", "partial-alpha"):
        img = _tiled(rng, w, h, _colors(rng, 300))
        img[img[..., 0] == 1] += np.array([1, 0, 0, 0], dtype=np.uint32)   # (no pixel shares the key's red by chance)
        if name != "partial-alpha":
            img[3, 4] = img[7, 1] = (1, 2, 3, 0)
        if name == "key-opaque-before":
            img[0, 0] = (1, 2, 3, 255)
        if name == "key-opaque-after":
            img[-1, -1] = (1, 2, 3, 255)
        if name == "key-two-rgbs":
            img[9, 9] = (1, 2, 4, 0)
        if name == "partial-alpha":
            img[5, 5, 3] = 128
        return img
    if name == "key-4x4":
        img = _colors(rng, 16).reshape(4, 4, 4)
        img[2, 1] = (1, 2, 3, 0)
        return img
    if name in ("grey-key", "grey-alpha"):
        g = rng.integers(8, 256, size=(h, w)).astype(np.uint32)
        a = np.full_like(g, 255)
        if name == "grey-key":
            g[2, 3], a[2, 3] = 7, 0
            g[h - 1, 0], a[h - 1, 0] = 7, 0
        else:
            a = rng.integers(0, 256, size=(h, w)).astype(np.uint32)
        return np.stack([g, g, g, a], axis=2)
    if kind.startswith("grey") and kind[4:].isdigit():
        return _grey_levels(rng, w, h, int(kind[4:]))
    if name in ("fake16", "fake16-last-low", "fake16-ga"):
        img = _tiled(rng, w, h, _colors(rng, 9)) * 257
        if name == "fake16-ga":
            img[..., 3] = (rng.integers(0, 4, size=(h, w)) * 85 * 257).astype(np.uint32)
        if name == "fake16-last-low":
            img[-1, -1, -1] ^= 1
        return img
    if name == "true16-grey":
        g = rng.integers(0, 65536, size=(h, w)).astype(np.uint32)
        return np.stack([g, g, g, np.full_like(g, 65535)], axis=2)
    if name in ("true16-rgb-key", "true16-rgba"):
        img = rng.integers(0, 65536, size=(h, w, 4)).astype(np.uint32)
        if name == "true16-rgb-key":
            img[..., 3] = 65535
            img[img[..., 0] == 0x0102] += np.array([1, 0, 0, 0], dtype=np.uint32)
            img[1, 1] = img[4, 2] = (0x0102, 0x0304, 0x0506, 0)
        return img
    if name == "few-pixels":
        return _tiled(rng, w, h, _colors(rng, 3))
    if name == "exactly-2n":
        return _tiled(rng, w, h, _colors(rng, 3))
    if name == "retry-40":
        y, x = np.mgrid[0:h, 0:w]
        k = (x + y * w) // 2
        return np.stack([40 + 3 * k, 90 + 2 * k, 200 - k, np.full_like(k, 255)], axis=2).astype(np.uint32)
    if name == "retry-100-alpha":
        # (every colour somewhere, in no order: with the first appearances in a run the RGBA file is the smaller one)
        colors = _colors(rng, 100, alpha=True)
        idx = rng.integers(0, 100, size=w * h)
        idx[rng.permutation(w * h)[:100]] = np.arange(100)
        return colors[idx].reshape(h, w, 4)
    if name == "unchanged":
        return rng.integers(0, 256, size=(h, w, 4)).astype(np.uint32)
    raise KeyError(name)


def _grey_cases():
    out = []
    cts = (6, 2, 0)
    k = 0
    for bits in (1, 2, 4, 8):
        for w in (1, 7, 8, 9, 37):
            out.append((f"grey{bits}-w{w}-ct{cts[k % 3]}", w, 5, cts[k % 3], 8))
            k += 1
        out.append((f"grey{bits}-w37-row", 37, 1, cts[k % 3], 8))
        out.append((f"grey{bits}-w1-column", 1, 23, cts[(k + 1) % 3], 8))
    return out


CASES = [
    ("colors-1", 8, 8, 6, 8), ("colors-2", 20, 10, 6, 8), ("colors-3", 20, 10, 2, 8), ("colors-4", 21, 11, 6, 8),
    ("colors-5", 21, 11, 6, 8), ("colors-16", 23, 9, 2, 8), ("colors-17", 23, 9, 6, 8), ("colors-256", 40, 30, 6, 8),
    ("colors-257", 40, 30, 6, 8), ("colors-256-spread", 300, 200, 6, 8), ("colors-last-pixel", 37, 19, 6, 8),
    ("colors-alpha-only", 19, 7, 6, 8), ("colors-00-ff", 15, 6, 6, 8), ("colors-257th-last", 40, 30, 2, 8),
    ("key", 30, 20, 6, 8), ("key-opaque-before", 30, 20, 6, 8), ("key-opaque-after", 30, 20, 6, 8), ("key-two-rgbs", 30, 20, 6, 8),
    ("partial-alpha", 30, 20, 6, 8), ("key-4x4", 4, 4, 6, 8), ("grey-key", 25, 12, 6, 8), ("grey-alpha", 25, 12, 6, 8),
] + _grey_cases() + [
    ("fake16", 13, 11, 6, 16), ("fake16-ga", 13, 11, 4, 16), ("fake16-last-low", 13, 11, 6, 16), ("true16-grey", 11, 9, 2, 16),
    ("true16-rgb-key", 12, 7, 6, 16), ("true16-rgba", 9, 8, 6, 16),
    ("few-pixels", 5, 1, 6, 8), ("exactly-2n", 3, 2, 6, 8),
    ("retry-40", 10, 8, 6, 8), ("retry-100-alpha", 16, 16, 6, 8),
    ("unchanged", 64, 33, 6, 8),
]
IDS = [c[0] for c in CASES]
_PIXELS = {}


def pixels(case):
    """(height, linebytes) uint8, PNG byte order; made once and never changed."""
    name, w, h, ct, depth = case
    if name not in _PIXELS:
        img = _bytes(_as(_make(name, w, h, ct, depth), ct), depth)
        img.setflags(write=False)
        _PIXELS[name] = img
    return _PIXELS[name]


_MODEL = {}


def model(case):
    """(rgba, stats, mode, converted) of a case, computed once."""
    name, w, h, ct, depth = case
    if name not in _MODEL:
        rgba = expand(pixels(case), w, h, ct, depth)
        st = stats(rgba, depth)
        mode = choose(st, w * h)
        _MODEL[name] = (rgba, st, mode, convert(rgba, depth, w, h, mode))
    return _MODEL[name]


# What every case has to reach: (colour type, bit depth, palette size, key, second try) — the second try None where
# zopflipng makes none (no palette, or a file of 4096 bytes or more), else whether it replaced the first file under
# strategy 0 and 2 iterations.  A case that ends elsewhere no longer tests its edge.
AS_IS = {"colors-257th-last", "key-opaque-before", "key-opaque-after", "key-two-rgbs", "partial-alpha", "key-4x4", "grey8-w8-ct0",
         "grey8-w37-row", "fake16-last-low", "true16-rgba", "unchanged"}   # the chosen mode is the image's own
_GREY = {f"grey{bits}-{tail}": (0, bits, 0, None, None) for bits in (1, 2, 4, 8)
         for tail in ("w1-ct", "w7-ct", "w8-ct", "w9-ct", "w37-ct", "w37-row", "w1-column")}
EXPECT = {
    "colors-1": (3, 1, 1, None, True),
    "colors-2": (3, 1, 2, None, False),
    "colors-3": (3, 2, 3, None, False),
    "colors-4": (3, 2, 4, None, False),
    "colors-5": (3, 4, 5, None, False),
    "colors-16": (3, 4, 16, None, False),
    "colors-17": (3, 8, 17, None, False),
    "colors-256": (3, 8, 256, None, False),
    "colors-257": (2, 8, 0, None, None),
    "colors-256-spread": (3, 8, 256, None, None),
    "colors-last-pixel": (3, 2, 3, None, False),
    "colors-alpha-only": (3, 4, 6, None, True),
    "colors-00-ff": (3, 2, 4, None, True),
    "colors-257th-last": (2, 8, 0, None, None),
    "key": (2, 8, 0, (1, 2, 3), None),
    "key-opaque-before": (6, 8, 0, None, None),
    "key-opaque-after": (6, 8, 0, None, None),
    "key-two-rgbs": (6, 8, 0, None, None),
    "partial-alpha": (6, 8, 0, None, None),
    "key-4x4": (6, 8, 0, None, None),
    "grey-key": (0, 8, 0, (7, 7, 7), None),
    "grey-alpha": (4, 8, 0, None, None),
    "fake16": (3, 4, 9, None, False),
    "fake16-ga": (3, 8, 31, None, True),
    "fake16-last-low": (6, 16, 0, None, None),
    "true16-grey": (0, 16, 0, None, None),
    "true16-rgb-key": (2, 16, 0, (258, 772, 1286), None),
    "true16-rgba": (6, 16, 0, None, None),
    "few-pixels": (2, 8, 0, None, None),
    "exactly-2n": (3, 2, 3, None, True),
    "retry-40": (3, 8, 40, None, True),
    "retry-100-alpha": (3, 8, 100, None, False),
    "unchanged": (6, 8, 0, None, None),
}
EXPECT.update({name: _GREY[name.rstrip("026")] for name in IDS if name.startswith("grey") and name[4].isdigit()})
