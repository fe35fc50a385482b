"""The images of zmx_png_encode_device's tests (tests/test_cpu_png_container.py, tests/test_gpu_png_encode.py) and the
PNG container in plain Python: ten small shapes over the four colour types at both depths, down to one row and one
column; a minimal PNG writer (zlib) for the reference's command line to read; the chunks of a file."""
import struct
import zlib

import numpy as np

CHANNELS = {0: 1, 2: 3, 4: 2, 6: 4}
# (width, height, colour type, bit depth)
SHAPES = [
    (37, 19, 2, 8),
    (64, 33, 6, 8),
    (31, 17, 0, 16),
    (17, 11, 6, 16),
    (5, 1, 2, 8),
    (1, 7, 6, 8),
    (50, 20, 0, 8),
    (23, 13, 4, 8),
    (12, 9, 2, 16),
    (9, 14, 4, 16),
]
WIDE = (600, 8, 6, 8)   # rows of 2400 bytes: LodePNG's window of 2048 and zopflipng's of 32768 see different matches
STRATEGY_LETTERS = {0: "0", 1: "1", 2: "2", 3: "3", 4: "4", 5: "m", 6: "e", 7: "b"}
PREDEFINED = 8


def shape_id(s):
    return f"{s[0]}x{s[1]}-ct{s[2]}-d{s[3]}"


def bytewidth(shape):
    return CHANNELS[shape[2]] * shape[3] // 8


def pixels(shape):
    """(height, linebytes) uint8 in PNG byte order: a gradient with a little noise, a flat patch and a noisy corner, so
    that the row searches have something to choose between."""
    w, h, ct, depth = shape
    n = w * bytewidth(shape)
    rng = np.random.default_rng(w * 1000 + h * 10 + ct + depth)
    y, x = np.mgrid[0:h, 0:n]
    img = (x * 5 // bytewidth(shape) + y * 3 + rng.integers(-2, 3, size=(h, n))) & 255
    img[: max(1, h // 3), : max(1, n // 2)] = 40
    img[h // 2:, n // 2:] = rng.integers(0, 256, size=(h - h // 2, n - n // 2))
    return img.astype(np.uint8)


def mixed_types(h):
    return ((np.arange(h) * 3 + 1) % 5).astype(np.uint8)


def chunk(tag, data):
    body = tag + data
    return struct.pack(">I", len(data)) + body + struct.pack(">I", zlib.crc32(body) & 0xffffffff)


def ihdr(shape):
    w, h, ct, depth = shape
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ct, 0, 0, 0))


def plain_png(shape, scanlines):
    """A valid PNG of the (height, 1 + linebytes) scanlines — filter type, filtered row — deflated by zlib: an input for
    zopflipng, whose --filters=p takes the types from it."""
    raw = bytes(scanlines.tobytes())
    return b"\x89PNG\r\n\x1a\n" + ihdr(shape) + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b"")


def assemble(shape, zlib_stream):
    """The file zmx_png_encode_device promises, around zopfli's zlib stream of the filtered scanlines (78 DA ...)."""
    assert zlib_stream[:2] == b"\x78\xda"
    return b"\x89PNG\r\n\x1a\n" + ihdr(shape) + chunk(b"IDAT", b"\x78\x01" + zlib_stream[2:]) + chunk(b"IEND", b"")


def chunks(png):
    """[(tag, data)] of a PNG file; the signature and every CRC are checked."""
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    out, at = [], 8
    while at < len(png):
        n, = struct.unpack(">I", png[at:at + 4])
        tag, data = png[at + 4:at + 8], png[at + 8:at + 8 + n]
        assert struct.unpack(">I", png[at + 8 + n:at + 12 + n])[0] == zlib.crc32(tag + data) & 0xffffffff
        out.append((tag, data))
        at += 12 + n
    assert at == len(png)
    return out
