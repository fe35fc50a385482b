"""Palette, 1/2/4-bit grey and index images in plain numpy, and the images the zmx_png_index_* entries are tested on
(tests/test_cpu_png_index_cases.py, tests/test_gpu_png_index.py, tests/golden/make_png_index_golden.py).

A case is (name, width, height, colour type, bit depth, palette); `values(case)` its (height, width) index values,
`packed(case)` the (height, linebytes) bytes as the entries take them — first pixel in a byte's top bits, GARBAGE in the
padding bits behind a row's last pixel.  The model: the first-appearance table, the palette the values stand for (the grey
ramp for colour type 0), the RGBA8 expansion zopflipng sees, its --lossy_transparent rewrite, the mode and table of the
--keepcolortype file, and the table-driven conversion.  png_color_cases' stats, choose, retry_mode, convert and assemble
say what LodePNG makes of the expansion."""
import zlib

import numpy as np

import png_color_cases as cc
from png_encode_cases import chunk

UNUSED = (1 << 64) - 1
LOSSY_TRANSPARENT = 1

BW = [(0, 0, 0, 255), (255, 255, 255, 255)]
TWO = [(200, 10, 10, 255), (10, 10, 200, 255)]
FOUR = [(200, 10, 10, 255), (10, 200, 10, 255), (10, 10, 200, 255), (250, 250, 5, 255)]
THREE = FOUR[:3]


def _many(n, alpha=False):
    """n distinct coloured entries, opaque unless `alpha`."""
    return [((37 * i + 11) % 256, (91 * i + 5) % 256, (53 * i + 200) % 256, (255 - 3 * i) if alpha and i % 3 else 255) for i in range(n)]


GREYS20 = [(8 + 11 * i,) * 3 + (255,) for i in range(20)]
SIXTEEN = _many(16)


def _shapes():
    out = []
    for h in (1, 3):
        for w in (1, 2, 3, 7, 8, 9, 15, 16, 17):
            kind = (w + h) % 3
            out.append((f"b1-w{w}-h{h}", w, h, 0 if kind == 0 else 3, 1, None if kind == 0 else (BW if kind == 1 else TWO)))
        for w in (1, 3, 4, 5):
            kind = (w + h) % 3
            out.append((f"b2-w{w}-h{h}", w, h, 0 if kind == 0 else 3, 2, None if kind == 0 else (FOUR if kind == 1 else THREE)))
        for w in (1, 2, 3):
            kind = (w + h) % 2
            out.append((f"b4-w{w}-h{h}", w, h, 0 if kind == 0 else 3, 4, None if kind == 0 else SIXTEEN[:11]))
    return out


CASES = _shapes() + [
    ("big1", 600, 300, 3, 1, BW),                      # several workgroups; grey at 1 bit from a black / white palette
    ("big8", 200, 100, 3, 8, _many(256)),              # ... all 256 values used, each in several workgroups' shares
    ("last-pixel", 37, 19, 3, 8, THREE),               # a value that first appears in the very last pixel; 8 bits -> 2
    ("two-equal", 5, 3, 3, 2, [FOUR[0], FOUR[1], FOUR[0], FOUR[2]]),   # both used, the later one first
    ("unused", 9, 4, 3, 4, _many(8)),                  # palettesize below 2^bitdepth, three entries used
    ("bw-8", 20, 10, 3, 8, BW),                        # grey at 1 bit
    ("grey8", 30, 20, 3, 8, [(3 + 6 * i,) * 3 + (255,) for i in range(40)]),
    ("grey-key", 25, 12, 3, 8, GREYS20 + [(7, 7, 7, 0)]),
    ("grey-key-16px", 4, 4, 3, 4, GREYS20[:8] + [(7, 7, 7, 0)]),
    ("few-rgb", 5, 1, 3, 2, THREE),
    ("few-rgba", 5, 1, 3, 2, [(200, 10, 10, 255), (10, 200, 10, 128), (10, 10, 200, 255)]),
    ("partial-alpha", 30, 20, 3, 8, _many(40, alpha=True)),
    ("two-transparent", 21, 11, 3, 4, [FOUR[0], (10, 20, 30, 0), FOUR[1], (40, 50, 60, 0), FOUR[2]]),
    ("one-transparent-first", 16, 5, 3, 2, [(9, 9, 9, 0), FOUR[0], FOUR[1]]),
    ("grey2-wide", 33, 7, 0, 2, None),
    ("grey4-wide", 33, 7, 0, 4, None),
]
IDS = [c[0] for c in CASES]
# the cases whose reference files are kept (tests/golden/png_index.json: small files, a few kilobytes in all)
GOLDEN_NAMES = ["b1-w17-h3", "b2-w5-h3", "b4-w2-h3", "two-equal", "unused", "grey-key-16px", "few-rgba", "two-transparent", "one-transparent-first"]
GOLDEN_AUTO = ["two-transparent"]   # ... also without --filters

# a value at or above palettesize: (case, the first such pixel)
OUTSIDE = [(("outside-4", 9, 4, 3, 4, _many(5)), 23), (("outside-1", 17, 3, 3, 1, BW[:1]), 40)]


def case(name):
    return CASES[IDS.index(name)]


SMALL = [case(n) for n in GOLDEN_NAMES]


def palette_of(c):
    """(n, 4) uint8: the entries the values stand for."""
    _, _, _, ct, depth, pal = c
    if ct == 3:
        return np.array(pal, dtype=np.uint8).reshape(-1, 4)
    g = (np.arange(1 << depth) * 255 // ((1 << depth) - 1)).astype(np.uint8)
    return np.stack([g, g, g, np.full_like(g, 255)], axis=1)


_VALUES = {}


def values(c):
    """(height, width) index values; made once and never changed."""
    name, w, h, ct, depth, pal = c
    if name in _VALUES:
        return _VALUES[name]
    rng = np.random.default_rng(sum(name.encode()) * 7919 + w * 31 + h)
    n = len(palette_of(c))
    if name == "last-pixel":
        v = rng.integers(0, 2, size=(h, w))
        v.flat[-1] = 2
    elif name == "two-equal":
        v = rng.integers(0, 4, size=(h, w))
        v.flat[:4] = (1, 2, 3, 0)
    elif name == "unused":
        v = rng.choice([1, 4, 6], size=(h, w))
    elif name == "big8":
        v = rng.integers(0, 256, size=(h, w))
        v.flat[:256] = rng.permutation(256)
    elif name == "grey-key":
        v = rng.integers(0, 20, size=(h, w))
        v[2, 3] = v[h - 1, 0] = 20
        v.flat[:20] = np.arange(20)
    elif name == "grey-key-16px":
        v = rng.integers(0, 8, size=(h, w))
        v.flat[:9] = np.arange(9)
    elif name == "two-transparent":
        v = rng.choice([0, 2, 4], size=(h, w))
        v[1, 5], v[0, 7], v[4, 4] = 1, 3, 3
    elif name == "one-transparent-first":
        v = rng.integers(0, 3, size=(h, w))
        v.flat[0] = 0
    elif name.startswith("outside"):
        v = rng.integers(0, n, size=(h, w))
        at = dict((k[0][0], k[1]) for k in OUTSIDE)[name]
        v.flat[at] = v.flat[-1] = (1 << depth) - 1
    else:
        v = rng.integers(0, n, size=(h, w))
        if w * h >= n:
            v.flat[rng.permutation(w * h)[:n]] = np.arange(n)   # every entry somewhere
    v = v.astype(np.uint8)
    v.setflags(write=False)
    _VALUES[name] = v
    return v


def pack(vals, depth, garbage=True):
    """(height, linebytes) uint8: `depth` bits a pixel, the first in a byte's top bits; the padding bits set unless not
    `garbage`."""
    h, w = vals.shape
    per = 8 // depth
    cols = -(-w // per) * per
    bits = np.ones((h, cols, depth), dtype=np.uint8) if garbage else np.zeros((h, cols, depth), dtype=np.uint8)
    bits[:, :w, :] = (vals[:, :, None] >> np.arange(depth - 1, -1, -1)) & 1
    return np.packbits(bits.reshape(h, -1), axis=1)


def packed(c):
    out = pack(values(c), c[4])
    out.setflags(write=False)
    return out


# ---- the model
def first_table(vals):
    """first[v]: the smallest raster index at which v occurs, UNUSED for a value no pixel has (256 Python integers)."""
    flat = np.asarray(vals).reshape(-1)
    out = [UNUSED] * 256
    u, at = np.unique(flat, return_index=True)
    for v, i in zip(u, at):
        out[int(v)] = int(i)
    return out


def expand(c, lossy=0):
    """(h * w, 4) uint32: the RGBA8 pixels zopflipng sees, after --lossy_transparent where asked: every pixel with alpha 0
    gets the RGB of the first one in raster order (an index image has at most 256 colours: always the palette mode)."""
    rgba = palette_of(c)[values(c).reshape(-1)].astype(np.uint32)
    if lossy & LOSSY_TRANSPARENT:
        clear = np.nonzero(rgba[:, 3] == 0)[0]
        if len(clear):
            rgba[clear, :3] = rgba[clear[0], :3]
    return rgba


def seen_palette(c, lossy=0):
    """The entries after --lossy_transparent: the used ones with alpha 0 carry the first transparent pixel's RGB."""
    pal = palette_of(c).copy()
    if lossy & LOSSY_TRANSPARENT:
        first = first_table(values(c))
        clear = [i for i in range(len(pal)) if first[i] != UNUSED and pal[i, 3] == 0]
        if clear:
            pal[clear, :3] = pal[min(clear, key=lambda i: first[i]), :3]
    return pal


def keep_mode(c, lossy=0):
    """The mode of zopflipng --keepcolortype's file: the input's, with its palette — after --lossy_transparent shrunk to the
    entries whose OWN colour still occurs where that leaves fewer colours than entries (zopflipng_lib.cc:137-155)."""
    _, _, _, ct, depth, _ = c
    if ct != 3:
        return {"colortype": 0, "bitdepth": depth, "palette": None, "key": None}
    pal = palette_of(c)
    if lossy & LOSSY_TRANSPARENT:
        occurs = {tuple(int(x) for x in px) for px in np.unique(expand(c, lossy), axis=0)}
        if len(occurs) < len(pal):
            pal = np.array([e for e in pal if tuple(int(x) for x in e) in occurs], dtype=np.uint8).reshape(-1, 4)
    return {"colortype": 3, "bitdepth": depth, "palette": pal, "key": None}


def table_for(pal, mode):
    """k_png_index_convert's 256 entries for the entries `pal` (n, 4) into `mode`: the first output byte lowest."""
    out = [0] * 256
    for i, e in enumerate(pal):
        r, g, b, a = (int(x) for x in e)
        ct = mode["colortype"]
        if ct == 3:
            v = 0
            for j, m in enumerate(np.asarray(mode["palette"])):
                if (r, g, b, a) == tuple(int(x) for x in m):
                    v = j
        elif ct == 0:
            v = r >> (8 - mode["bitdepth"])
        elif ct == 4:
            v = r | (a << 8)
        elif ct == 2:
            v = r | (g << 8) | (b << 16)
        else:
            v = r | (g << 8) | (b << 16) | (a << 24)
        out[i] = v
    return out


def convert_table(vals, table, mode):
    """(h, rowbytes) uint8: the values through `table` in `mode`; rows packed most significant bits first, padded with zeros."""
    h, w = vals.shape
    e = np.array(table, dtype=np.uint32)[vals]
    bpp = cc.bpp(mode)
    if bpp < 8:
        return pack((e & ((1 << bpp) - 1)).astype(np.uint8), bpp, garbage=False)
    return ((e[:, :, None] >> (8 * np.arange(bpp // 8))) & 255).astype(np.uint8).reshape(h, -1)


# ---- an input for the reference's command line
def input_png(c):
    """A PNG of the case as it is: IHDR, PLTE and tRNS for a palette, one IDAT of unfiltered rows (padding bits zero)."""
    name, w, h, ct, depth, _ = c
    mode = {"colortype": ct, "bitdepth": depth, "palette": palette_of(c) if ct == 3 else None, "key": None}
    rows = pack(values(c), depth, garbage=False)
    scan = np.concatenate([np.zeros((h, 1), dtype=np.uint8), rows], axis=1)
    return b"\x89PNG\r\n\x1a\n" + cc.ihdr(w, h, mode) + cc.color_chunks(mode) + chunk(b"IDAT", zlib.compress(scan.tobytes(), 6)) + chunk(b"IEND", b"")


# What every named case has to reach without --keepcolortype: (colour type, bit depth, palette size, key); a case that
# ends elsewhere no longer tests its edge.  With --lossy_transparent where it differs: LOSSY_EXPECT.
EXPECT = {
    "big1": (0, 1, 0, None),
    "big8": (3, 8, 256, None),
    "last-pixel": (3, 2, 3, None),
    "two-equal": (3, 2, 3, None),
    "unused": (3, 2, 3, None),
    "bw-8": (0, 1, 0, None),
    "grey8": (0, 8, 0, None),
    "grey-key": (0, 8, 0, (7, 7, 7)),
    "grey-key-16px": (4, 8, 0, None),
    "few-rgb": (2, 8, 0, None),
    "few-rgba": (6, 8, 0, None),
    "partial-alpha": (3, 8, 40, None),
    "two-transparent": (3, 4, 5, None),
    "one-transparent-first": (3, 2, 3, None),
    "grey2-wide": (0, 2, 0, None),
    "grey4-wide": (0, 4, 0, None),
}
LOSSY_EXPECT = {"two-transparent": (3, 2, 4, None)}
# the --keepcolortype file's palette size: without, with --lossy_transparent
KEEP_PALETTE = {"two-equal": (4, 4), "unused": (8, 3), "two-transparent": (5, 4), "one-transparent-first": (3, 3), "big8": (256, 256)}


def mode_tuple(mode):
    return (mode["colortype"], mode["bitdepth"], 0 if mode["palette"] is None else len(mode["palette"]), mode["key"])
