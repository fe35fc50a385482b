"""The PNG row filters in plain numpy and the case table of zmx_png_filter_rows_device's tests:
tests/test_cpu_png_rows_cases.py holds the reference against LodePNG's own filter and runs the table through the
header's rules on the CPU (tests/hostlib/png_rows_print.cc), tests/test_gpu_png_rows.py through k_png_rows.  A case is
an image of `height` rows of `linebytes` bytes, the distance `bytewidth` to a byte's left neighbour (it divides
linebytes, so that LodePNG can be asked about the same image) and a filter type for every row."""
import zlib

import numpy as np

GUARD = 64          # bytes of 0xA5 on both sides of the output
THREADS = 256       # zamd::kPngRowsThreads
MAX_BLOCKS = 2048   # zamd::kPngRowsMaxBlocks
BYTEWIDTHS = (1, 2, 3, 4, 6, 8)
# (colour type, bit depth) of an image whose pixels are `bytewidth` bytes: what LodePNG is told
LODEPNG_MODE = {1: (0, 8), 2: (0, 16), 3: (2, 8), 4: (6, 8), 6: (2, 16), 8: (6, 16)}


def filter_rows(img, bytewidth, types):
    """The scanlines LodePNG's encoder hands to its deflate (lodepng.cpp filterScanline): row r is types[r] followed by
    the row filtered that way — 0 None, 1 Sub, 2 Up, 3 Average (the 9-bit sum halved), 4 Paeth (the PNG specification's
    predictor: a on pa <= pb and pa <= pc, else b on pb <= pc, else c).  Zeros above row 0 and left of a row's first
    `bytewidth` bytes."""
    img = np.asarray(img, dtype=np.uint8)
    h, n = img.shape
    types = np.asarray(types, dtype=np.uint8)
    assert types.shape == (h,) and types.max(initial=0) <= 4
    s = img.astype(np.int32)
    a = np.zeros_like(s)
    b = np.zeros_like(s)
    c = np.zeros_like(s)
    if bytewidth < n:
        a[:, bytewidth:] = s[:, :n - bytewidth]
        c[1:, bytewidth:] = s[:-1, :n - bytewidth]
    b[1:] = s[:-1]
    pa, pb, pc = np.abs(b - c), np.abs(a - c), np.abs(a + b - 2 * c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    by_type = [s, s - a, s - b, s - ((a + b) >> 1), s - paeth]
    out = np.empty((h, n + 1), dtype=np.uint8)
    out[:, 0] = types
    t = types[:, None]
    data = np.zeros_like(s)
    for k in range(5):
        data = np.where(t == k, by_type[k], data)
    out[:, 1:] = (data & 255).astype(np.uint8)
    return out


def grid(total):
    """zamd::PngRowsGrid"""
    return min(max((total // 16 + THREADS - 1) // THREADS, 1), MAX_BLOCKS)


def _pixels(kind, rng, h, n):
    if kind == "noise":
        return rng.integers(0, 256, size=(h, n), dtype=np.uint8)
    if kind == "ones":          # 255 + 255: the ninth bit of Average's sum
        return np.full((h, n), 255, dtype=np.uint8)
    if kind == "ties":          # few values, near each other and at both ends: pa == pb, pb == pc, pa == pc all occur
        return rng.choice(np.array([0, 1, 2, 3, 127, 128, 129, 254, 255], dtype=np.uint8), size=(h, n))
    if kind == "gradient":
        y, x = np.mgrid[0:h, 0:n]
        return ((x * 3 + y * 2 + rng.integers(-2, 3, size=(h, n))) & 255).astype(np.uint8)
    raise ValueError(kind)


def _types(how, h, shift):
    if how == "cycle":          # neighbouring rows differ
        return ((np.arange(h) + shift) % 5).astype(np.uint8)
    return np.full(h, int(how), dtype=np.uint8)


def _table():
    out = []
    # every row length up to 40: a 16-byte vector of the output spans up to 8 rows
    for n in range(1, 41):
        divisors = [b for b in BYTEWIDTHS if n % b == 0]
        out.append((f"short-{n}", n, 9, divisors[n % len(divisors)], "noise", "cycle"))
    # around the vector, a wave's and a workgroup's share; every pixel size at a long row
    for n, bw in ((63, 3), (64, 8), (65, 1), (1023, 3), (1024, 2), (1025, 1), (4095, 3), (4097, 1), (4098, 6), (1024, 4),
                  (1024, 8), (1026, 6)):
        out.append((f"long-{n}-bw{bw}", n, 6, bw, "noise", "cycle"))
    for t in range(5):
        out.append((f"one-row-type{t}", 100, 1, 4, "noise", str(t)))
    for bw in BYTEWIDTHS:       # one pixel a row: no byte has a left neighbour
        out.append((f"width-1-bw{bw}", bw, 7, bw, "noise", "cycle"))
    out.append(("ones-bw1", 70, 6, 1, "ones", "cycle"))
    out.append(("ones-bw4", 72, 6, 4, "ones", "3"))
    out.append(("ties-bw1", 67, 12, 1, "ties", "4"))
    out.append(("ties-bw3", 66, 12, 3, "ties", "cycle"))
    out.append(("gradient", 300, 40, 3, "gradient", "cycle"))
    for t in range(5):
        out.append((f"noise-type{t}", 257 * 4, 33, 4, "noise", str(t)))
    out.append(("blocks", 4097, 40, 1, "noise", "cycle"))            # some forty workgroups
    return out


TABLE = _table()
# more output than one sweep of the capped grid writes (2048 workgroups of 256 vectors of 16 bytes): the threads stride
BIG = ("stride", 8196, 1100, 4, "noise", "cycle")


def make(case):
    """(image (height, linebytes) uint8, types (height,) uint8) of a row of the table; the bytes depend on its name alone."""
    name, n, h, _, kind, how = case
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    return _pixels(kind, rng, h, n), _types(how, h, zlib.crc32(name.encode()) % 5)
