"""SURVEY 8 f-3 on the GPU, the brute-force strategy: zmx_png_filter_types_brute (k_png_brute) against LodePNG's own
LFS_BRUTE_FORCE search (lodepng.cpp:5585-5632) at its default window of 2048, and libzopflipng_amd.so with
`--filters=b` against the reference's zopflipng (window 32768), file for file and row for row.

The CPU reference only runs here on inputs where its brute search takes about a second or less on the build host
(<= 1024 x 64 at window 2048, <= 256 x 256 RGBA at window 32768); the 1024 x 1024 image comes from
tests/golden/png_brute.json (tools/png_brute.py --make-golden)."""
import ctypes
import hashlib
import json
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from zopfli_amd import Context

pytestmark = pytest.mark.gpu

LFS_BRUTE_FORCE = 7      # lodepng.h:680-698
LCT_GREY, LCT_RGB, LCT_PALETTE, LCT_GREY_ALPHA, LCT_RGBA = 0, 2, 3, 4, 6
ZMX_ERR_REFUSED = 3      # include/zopfli_amd.h


def _filter_ref():
    from zopfli_amd._build import PNG_FILTER_REF
    assert os.path.exists(PNG_FILTER_REF), "oracle/_ref/libpng_filter_ref.so not built"
    lib = ctypes.CDLL(PNG_FILTER_REF)
    lib.ref_png_filter.argtypes = [ctypes.c_char_p, ctypes.c_char_p] + [ctypes.c_uint] * 5
    lib.ref_png_filter.restype = ctypes.c_uint
    return lib


def _brute(gpu_lib, ctx, raw, linebytes, h, bytewidth, window):
    fn = gpu_lib.zmx_png_filter_types_brute
    fn.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint,
                   ctypes.c_void_p]
    fn.restype = ctypes.c_int
    out = np.full(max(h, 1), 255, dtype=np.uint8)
    rc = fn(ctx.handle, raw, linebytes, h, bytewidth, window, out.ctypes.data)
    return rc, out[:h]


def _image(rng, w, h, channels, depth, kind):
    """Raw scanlines (h rows of linebytes bytes): a gradient with a little noise, flat colour with rare changes, noise,
    or a gradient with transparent (all-zero) areas and whole zero rows."""
    bpp = channels * depth
    linebytes = (w * bpp + 7) // 8
    if kind == "noise":
        return rng.integers(0, 256, size=(h, linebytes), dtype=np.uint8), linebytes
    if kind == "flat":
        img = np.full((h, linebytes), 17, dtype=np.uint8)
        for _ in range(max(1, h // 3)):
            img[rng.integers(0, h), rng.integers(0, linebytes)] = rng.integers(0, 256)
        img[h // 2:] = 0
        return img, linebytes
    y, x = np.mgrid[0:h, 0:linebytes]
    img = ((x * 3 // max(1, bpp // 8 if bpp >= 8 else 1) + y * 2 + rng.integers(-2, 3, size=(h, linebytes))) & 255).astype(np.uint8)
    if kind == "zeros":
        px = max(1, bpp // 8)
        for r in range(h):
            if r % 5 == 2:
                img[r] = 0
                continue
            a, b = sorted(rng.integers(0, w + 1, size=2))
            img[r, a * px:b * px] = 0
            img[r, (w // 3) * px:(w // 3 + 7) * px] = 0
    return img, linebytes


CASES = [
    # (w, h, colortype, channels, bitdepth, kind): the 11 geometries of test_gpu_png.py
    (257, 33, LCT_RGBA, 4, 8, "gradient"),
    (1024, 64, LCT_RGBA, 4, 8, "gradient"),      # 4096-byte rows: the 2048 window wraps
    (300, 40, LCT_RGB, 3, 8, "gradient"),
    (513, 20, LCT_GREY, 1, 8, "gradient"),
    (129, 17, LCT_GREY, 1, 16, "gradient"),
    (77, 19, LCT_RGBA, 4, 16, "noise"),
    (1001, 9, LCT_GREY, 1, 4, "gradient"),
    (333, 11, LCT_PALETTE, 1, 2, "noise"),
    (64, 50, LCT_RGBA, 4, 8, "flat"),
    (5, 1, LCT_RGB, 3, 8, "noise"),
    (4096, 3, LCT_GREY_ALPHA, 2, 8, "gradient"),
    # and the brute search's own corners
    (300, 25, LCT_RGBA, 4, 8, "zeros"),          # transparent areas: the chainz walk and the zero skip
    (1024, 20, LCT_RGBA, 4, 8, "zeros"),         # ... in rows longer than the window
    (700, 12, LCT_RGBA, 4, 8, "flat"),           # long flat runs: matches >= nicematch and of 258
    (1024, 8, LCT_RGBA, 4, 8, "noise"),          # short chains, stale links after the wrap
    (1, 9, LCT_GREY, 1, 8, "gradient"),          # rows of 1 byte
    (1, 7, LCT_GREY_ALPHA, 2, 8, "noise"),       # rows of 2 bytes
]


def _case_id(c):
    return f"{c[0]}x{c[1]}-ct{c[2]}-d{c[4]}-{c[5]}"


def _vs_lodepng(gpu_lib, raw, w, h, colortype, depth, bytewidth, linebytes):
    ref = _filter_ref()
    out = ctypes.create_string_buffer(h * (linebytes + 1))
    assert ref.ref_png_filter(out, raw, w, h, colortype, depth, LFS_BRUTE_FORCE) == 0
    want = np.frombuffer(out.raw, dtype=np.uint8).reshape(h, linebytes + 1)[:, 0].copy()
    ctx = Context(0, gpu_lib)
    try:
        rc, got = _brute(gpu_lib, ctx, raw, linebytes, h, bytewidth, 2048)
        assert rc == 0, ctx.error()
    finally:
        ctx.close()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"rows {bad[:10].tolist()}: device {got[bad[:10]].tolist()} LodePNG {want[bad[:10]].tolist()}"


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_png_brute_vs_lodepng(gpu_lib, case):
    """zmx_png_filter_types_brute(..., 2048) == the filter type byte LodePNG's filter() with LFS_BRUTE_FORCE (window
    2048, its default) puts in front of every scanline: 8- and 16-bit, packed, one-row, zero-heavy, flat, wrapping and
    1- and 2-byte rows."""
    w, h, colortype, channels, depth, kind = case
    rng = np.random.default_rng(w * 131 + h)
    img, linebytes = _image(rng, w, h, channels, depth, kind)
    _vs_lodepng(gpu_lib, img.tobytes(), w, h, colortype, depth, (channels * depth + 7) // 8, linebytes)


# Two RGBA rows of 5 pixels (found with tools/models/png_brute_model.cc): on the second row Up (2) and Paeth (4) both
# compress to 23 bytes, in 131 and 130 bits of deflate data; LodePNG compares bytes and keeps the first, Up.
TIE_PREV = [180, 0, 120, 180, 0, 0, 0, 0, 60, 120, 0, 120, 0, 180, 180, 60, 60, 0, 60, 180]
TIE_ROW = [180, 2, 121, 181, 1, 0, 2, 0, 62, 121, 2, 121, 1, 180, 181, 62, 62, 1, 61, 181]


def test_png_brute_tie_in_bytes_not_bits(gpu_lib):
    """Types that tie in bytes but not in bits: the first of them wins, as in LodePNG (lodepng.cpp:5621)."""
    raw = bytes(TIE_PREV + TIE_ROW)
    _vs_lodepng(gpu_lib, raw, 5, 2, LCT_RGBA, 8, 4, 20)
    ctx = Context(0, gpu_lib)
    try:
        rc, got = _brute(gpu_lib, ctx, raw, 20, 2, 4, 2048)
        assert rc == 0, ctx.error()
    finally:
        ctx.close()
    assert got[1] == 2


def test_png_brute_refusals(gpu_lib):
    """A window of 0, 3 or 65536 is refused (ZMX_ERR_REFUSED; LodePNG's errors 60 / 90); height 0 returns 0."""
    raw = bytes(range(64))
    ctx = Context(0, gpu_lib)
    try:
        for window in (3, 65536, 0):
            rc, _ = _brute(gpu_lib, ctx, raw, 16, 4, 4, window)
            assert rc != 0, window
            assert gpu_lib.zmx_last_error_class() == ZMX_ERR_REFUSED, (window, ctx.error())
        rc, _ = _brute(gpu_lib, ctx, raw, 16, 0, 4, 32768)
        assert rc == 0, ctx.error()
    finally:
        ctx.close()


# ---- libzopflipng_amd.so against the reference's zopflipng (window 32768)

def _chunk(tag, data):
    body = tag + data
    return struct.pack(">I", len(data)) + body + struct.pack(">I", zlib.crc32(body) & 0xffffffff)


def _png(path, w, h, colortype, depth, rows, plte=None):
    raw = b"".join(b"\x00" + bytes(r) for r in rows)
    png = b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, colortype, 0, 0, 0))
    if plte is not None:
        png += _chunk(b"PLTE", plte)
    png += _chunk(b"IDAT", zlib.compress(raw, 6)) + _chunk(b"IEND", b"")
    with open(path, "wb") as f:
        f.write(png)


def _rgba_pixels():
    """200 x 120 RGBA, more than 256 colours and varied alpha (LodePNG keeps it RGBA 8: its raw rows are these bytes),
    a fully transparent corner."""
    rng = np.random.default_rng(11)
    w, h = 200, 120
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([x * 255 // (w - 1), y * 255 // (h - 1), (x + y) // 3 % 256, (x * 2 + y) % 256], axis=-1).astype(np.int32)
    img[..., :3] += rng.integers(-3, 4, size=(h, w, 3))
    img = np.clip(img, 0, 255).astype(np.uint8)
    img[:30, :40] = 0
    return img


def _make_inputs(tmp_path):
    rng = np.random.default_rng(5)
    files = {}
    img = _rgba_pixels()
    files["rgba"] = str(tmp_path / "rgba.png")
    _png(files["rgba"], img.shape[1], img.shape[0], LCT_RGBA, 8, img.reshape(img.shape[0], -1))
    w, h = 301, 77
    idx = ((np.mgrid[0:h, 0:w][1] // 7 + np.mgrid[0:h, 0:w][0] // 5) % 12).astype(np.uint8)
    packed = np.zeros((h, (w + 1) // 2), dtype=np.uint8)
    packed[:, :w // 2] = (idx[:, 0:w - 1:2] << 4) | idx[:, 1:w:2]
    packed[:, -1] = idx[:, -1] << 4
    files["pal"] = str(tmp_path / "pal.png")
    _png(files["pal"], w, h, LCT_PALETTE, 4, packed, plte=bytes(rng.integers(0, 256, size=36, dtype=np.uint8)))
    w, h = 90, 60
    g = (np.mgrid[0:h, 0:w][0] * 700 + np.mgrid[0:h, 0:w][1] * 300 + rng.integers(0, 50, size=(h, w))).astype(">u2")
    files["g16"] = str(tmp_path / "g16.png")
    _png(files["g16"], w, h, LCT_GREY, 16, g.view(np.uint8).reshape(h, w * 2))
    files["tiny"] = str(tmp_path / "tiny.png")
    _png(files["tiny"], 6, 5, LCT_RGB, 8, rng.integers(0, 2, size=(5, 18), dtype=np.uint8) * 255)
    return files


def _filter_bytes(png):
    """IHDR (w, h, depth, colour type) and the filter-type byte of every row of a non-interlaced PNG."""
    pos, idat, ihdr = 8, b"", None
    while pos < len(png):
        n = struct.unpack(">I", png[pos:pos + 4])[0]
        tag, data = png[pos + 4:pos + 8], png[pos + 8:pos + 8 + n]
        if tag == b"IHDR":
            ihdr = struct.unpack(">IIBB", data[:10])
            assert data[12] == 0, "interlaced"
        elif tag == b"IDAT":
            idat += data
        pos += 12 + n
    w, h, depth, ct = ihdr
    line = (w * {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[ct] * depth + 7) // 8 + 1
    rows = zlib.decompress(idat)
    assert len(rows) == h * line
    return ihdr, np.frombuffer(rows, dtype=np.uint8).reshape(h, line)[:, 0].copy()


def _run(exe, args, src, dst, env=None):
    r = subprocess.run([exe, "-y"] + args + [src, dst], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, (exe, r.stdout[-1000:], r.stderr[-1000:])
    with open(dst, "rb") as f:
        return f.read()


RUNS = [
    ("rgba", ["--iterations=1", "--filters=b"]),
    ("g16", ["--iterations=1", "--filters=b"]),
    ("pal", ["--iterations=1", "--filters=b"]),
    ("tiny", ["--iterations=1", "--filters=b"]),
    ("rgba", ["--iterations=1", "--filters=0meb"]),
    ("rgba", ["--iterations=1", "--filters=01234mepb"]),
]


@pytest.mark.parametrize("which,args", RUNS, ids=lambda v: v if isinstance(v, str) else "_".join(a.lstrip("-") for a in v))
def test_zopflipng_brute_vs_reference(gpu_lib, tmp_path, which, args):
    """The reference's zopflipng command line on libzopflipng_amd.so (brute-force row search on the device, window
    32768) writes the reference's PNG byte for byte; on the RGBA image the filter byte of every row of the reference's
    `--filters=b` output is zmx_png_filter_types_brute(..., 32768) of its raw rows."""
    from zopfli_amd._build import PNG_AMD2, PNG_REF
    assert os.path.exists(PNG_AMD2) and os.path.exists(PNG_REF), "oracle/_ref/zopflipng_amd2 / zopflipng_ref not built"
    src = _make_inputs(tmp_path)[which]
    ref = _run(PNG_REF, args, src, str(tmp_path / "ref.png"))
    if which == "rgba" and args[-1] == "--filters=b":
        (w, h, depth, ct), want = _filter_bytes(ref)
        assert (depth, ct) == (8, LCT_RGBA)
        img = _rgba_pixels()
        ctx = Context(0, gpu_lib)
        try:
            rc, got = _brute(gpu_lib, ctx, img.tobytes(), w * 4, h, 4, 32768)
            assert rc == 0, ctx.error()
        finally:
            ctx.close()
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, f"rows {bad[:10].tolist()}: device {got[bad[:10]].tolist()} reference {want[bad[:10]].tolist()}"
    amd = _run(PNG_AMD2, args, src, str(tmp_path / "amd.png"))
    assert amd == ref


def test_zopflipng_brute_host_filters_same_file(tmp_path):
    """--filters=b writes the same file with the device's search and with LodePNG's own (ZOPFLIPNG_AMD_HOST_FILTERS=1)."""
    from zopfli_amd._build import PNG_AMD2
    assert os.path.exists(PNG_AMD2), "oracle/_ref/zopflipng_amd2 not built"
    src = _make_inputs(tmp_path)["rgba"]
    dev = _run(PNG_AMD2, ["--iterations=1", "--filters=b"], src, str(tmp_path / "dev.png"))
    host = _run(PNG_AMD2, ["--iterations=1", "--filters=b"], src, str(tmp_path / "host.png"), {"ZOPFLIPNG_AMD_HOST_FILTERS": "1"})
    assert dev == host


def _at_size_png(path, w):
    """tools/png_at_size.py's synthetic W x W RGBA image (repeated here so that the test reads no file outside tests/):
    a gradient with +-3 of noise, seed 7, alpha 255 (LodePNG writes it as RGB)."""
    rng = np.random.default_rng(7)
    y, x = np.mgrid[0:w, 0:w]
    img = np.stack([(x * 255 // max(w - 1, 1)), (y * 255 // max(w - 1, 1)), ((x + y) // 3 % 256),
                    np.full_like(x, 255)], axis=-1).astype(np.int32)
    img[..., :3] += rng.integers(-3, 4, size=(w, w, 3))
    img = np.clip(img, 0, 255).astype(np.uint8)
    raw = np.concatenate([np.zeros((w, 1), dtype=np.uint8), img.reshape(w, w * 4)], axis=1).tobytes()
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, w, 8, 6, 0, 0, 0))
                + _chunk(b"IDAT", zlib.compress(raw, 1)) + _chunk(b"IEND", b""))
    return img


def test_zopflipng_brute_at_size_vs_golden(gpu_lib, tmp_path):
    """The 1024 x 1024 image with --filters=b --iterations=1: the output's SHA-256 and size and the 1024 filter types
    are the all-reference zopflipng's (tests/golden/png_brute.json, tools/png_brute.py --make-golden), and the device's
    search on the raw (RGB) rows gives the same types."""
    from zopfli_amd._build import PNG_AMD2
    assert os.path.exists(PNG_AMD2), "oracle/_ref/zopflipng_amd2 not built"
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png_brute.json")) as f:
        gold = json.load(f)["1024"]
    src = str(tmp_path / "in.png")
    img = _at_size_png(src, 1024)
    with open(src, "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == gold["input_sha256"], "the synthetic input is not the golden's"
    want = np.frombuffer(bytes.fromhex(gold["filter_types"]), dtype=np.uint8)
    rgb = np.ascontiguousarray(img[..., :3]).tobytes()
    ctx = Context(0, gpu_lib)
    try:
        rc, got = _brute(gpu_lib, ctx, rgb, 1024 * 3, 1024, 3, 32768)
        assert rc == 0, ctx.error()
    finally:
        ctx.close()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"rows {bad[:10].tolist()}: device {got[bad[:10]].tolist()} reference {want[bad[:10]].tolist()}"
    out = _run(PNG_AMD2, ["--filters=b", "--iterations=1"], src, str(tmp_path / "out.png"))
    (w, h, depth, ct), types = _filter_bytes(out)
    assert (w, h, depth, ct) == (1024, 1024, 8, LCT_RGB)
    assert np.array_equal(types, want)
    assert len(out) == gold["bytes"]
    assert hashlib.sha256(out).hexdigest() == gold["sha256"]
