"""zmx_png_color_stats_device and zmx_png_convert_device on the device: LodePNG's colour statistics and colour conversion
of an image in device memory, held against the numpy model of tests/png_color_cases.py (which
tests/test_cpu_png_color_cases.py holds against the all-reference zopflipng) on every case of its table.  The converted
image is written at two alignments of the destination between guard bytes; the image stays as it was; the statistics
are the same from run to run.  Every refusal leaves its output untouched."""
import ctypes

import numpy as np
import pytest
import torch

import png_color_cases as cc
from zopfli_amd import Context, api

pytestmark = pytest.mark.gpu

ZMX_ERR_REFUSED = 3
GUARD = 64


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    c = Context(0, gpu_lib)
    yield c
    c.close()


def _stats_dict(s):
    return {"colored": bool(s.colored), "key": bool(s.key), "alpha": bool(s.alpha), "numcolors": int(s.numcolors), "bits": int(s.bits),
            "key_rgb": (int(s.key_r), int(s.key_g), int(s.key_b)), "palette": np.array(s.colors(), dtype=np.uint8).reshape(-1, 4)}


def _mode_dict(m):
    return {"colortype": int(m.colortype), "bitdepth": int(m.bitdepth),
            "palette": np.array(m.colors(), dtype=np.uint8).reshape(-1, 4) if m.colortype == 3 else None,
            "key": (int(m.key_r), int(m.key_g), int(m.key_b)) if m.key_defined else None}


def mode_struct(mode):
    """The zmx_png_color_mode of a model mode."""
    m = api.PngColorMode()
    m.colortype, m.bitdepth = mode["colortype"], mode["bitdepth"]
    if mode["palette"] is not None:
        pal = np.asarray(mode["palette"], dtype=np.uint8)
        m.palettesize = len(pal)
        ctypes.memmove(m.palette, pal.tobytes(), 4 * len(pal))
    if mode["key"] is not None:
        m.key_defined = 1
        m.key_r, m.key_g, m.key_b = mode["key"]
    return m


def _same_mode(a, b):
    if (a["colortype"], a["bitdepth"], a["key"]) != (b["colortype"], b["bitdepth"], b["key"]):
        return False
    return (a["palette"] is None and b["palette"] is None) or np.array_equal(a["palette"], b["palette"])


def _convert(ctx, image, mode, total, offset):
    """The converted bytes written `offset` bytes behind a 256-byte boundary, and whether the guards held."""
    buf = torch.full((GUARD + 16 + total + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    at = GUARD + offset
    ctx.png_convert_device(image, mode_struct(mode), buf.data_ptr() + at, total)
    host = buf.cpu().numpy()
    return host[at:at + total], bool(np.all(host[:at] == 0xA5) and np.all(host[at + total:] == 0xA5))


@pytest.mark.parametrize("case", cc.CASES, ids=cc.IDS)
def test_stats_and_convert(ctx, gpu_lib, case):
    name, w, h, ct, depth = case
    img = cc.pixels(case)
    rgba, st, mode, conv = cc.model(case)
    d_img = torch.from_numpy(img.copy()).cuda()
    torch.cuda.synchronize()
    image = (d_img.data_ptr(), w, h, ct, depth)
    stats = ctx.png_color_stats_device(image)
    got = _stats_dict(stats)
    assert all(got[k] == st[k] for k in ("colored", "key", "alpha", "numcolors", "bits", "key_rgb")), (name, got, st)
    assert np.array_equal(got["palette"], st["palette"]), name
    assert bytes(stats.palette)[4 * len(st["palette"]):] == bytes(1024 - 4 * len(st["palette"])), "bytes behind the palette"
    again = ctx.png_color_stats_device(image)
    assert bytes(again) == bytes(stats), "the statistics differ from run to run"
    assert _same_mode(_mode_dict(api.png_choose_color(stats, w * h, lib=gpu_lib)), mode), name
    modes = [mode] + ([cc.retry_mode(st, w * h)] if mode["colortype"] == 3 else [])
    for m in modes:
        want = cc.convert(rgba, depth, w, h, m)
        for offset in (0, 5):
            out, guards = _convert(ctx, image, m, want.size, offset)
            assert guards, (name, offset, "written outside the output")
            assert np.array_equal(out, want.reshape(-1)), (name, m["colortype"], m["bitdepth"], offset)
    assert np.array_equal(d_img.cpu().numpy(), img), "the image changed"


def test_unaligned_image(ctx):
    """An image that starts 1, 4 and 8 bytes behind a 16-byte boundary: the byte, word and vector loads."""
    case = cc.CASES[cc.IDS.index("colors-17")]
    name, w, h, ct, depth = case
    img = cc.pixels(case)
    rgba, st, mode, conv = cc.model(case)
    for shift in (1, 4, 8, 16):
        buf = torch.zeros(img.size + 32, dtype=torch.uint8, device="cuda:0")
        buf[shift:shift + img.size] = torch.from_numpy(img.copy().reshape(-1)).cuda()
        torch.cuda.synchronize()
        image = (buf.data_ptr() + shift, w, h, ct, depth)
        got = _stats_dict(ctx.png_color_stats_device(image))
        assert got["numcolors"] == 17 and np.array_equal(got["palette"], st["palette"]), shift
        out, guards = _convert(ctx, image, mode, conv.size, 3)
        assert guards and np.array_equal(out, conv.reshape(-1)), shift


def test_colour_missing_from_the_palette(ctx, gpu_lib):
    """A caller's palette that lacks a colour of the image: the call fails and names the first such pixel."""
    case = cc.CASES[cc.IDS.index("colors-5")]
    name, w, h, ct, depth = case
    rgba, st, mode, conv = cc.model(case)
    d_img = torch.from_numpy(cc.pixels(case).copy()).cuda()
    out = torch.zeros(conv.size, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    short = dict(mode, palette=mode["palette"][[0, 1, 2, 4]])   # the fourth colour to appear is gone
    packed = [tuple(int(x) for x in px) for px in rgba]
    first = packed.index(tuple(int(x) for x in mode["palette"][3]))
    with pytest.raises(RuntimeError, match=rf"pixel {first} "):
        ctx.png_convert_device((d_img.data_ptr(), w, h, ct, depth), mode_struct(short), out)
    assert gpu_lib.zmx_last_error_class() == ZMX_ERR_REFUSED


def test_refusals_write_nothing(ctx, gpu_lib):
    lib = gpu_lib
    d_img = torch.zeros(64 * 64 * 8, dtype=torch.uint8, device="cuda:0")
    d_out = torch.full((64 * 64 * 8,), 0xA5, dtype=torch.uint8, device="cuda:0")
    on_host = np.zeros(4096, dtype=np.uint8)
    torch.cuda.synchronize()
    p, q = d_img.data_ptr(), d_out.data_ptr()
    fs = lib.zmx_png_color_stats_device
    fs.argtypes = [ctypes.c_void_p, ctypes.POINTER(api.PngImage), ctypes.POINTER(api.PngColorStats)]
    fs.restype = ctypes.c_int
    fc = lib.zmx_png_convert_device
    fc.argtypes = [ctypes.c_void_p, ctypes.POINTER(api.PngImage), ctypes.POINTER(api.PngColorMode), ctypes.c_void_p, ctypes.c_size_t]
    fc.restype = ctypes.c_int
    bad_images = [
        ("width 0", (p, 0, 16, 6, 8)),
        ("height 0", (p, 16, 0, 6, 8)),
        ("palette input", (p, 16, 16, 3, 8)),
        ("colour type 1", (p, 16, 16, 1, 8)),
        ("depth 4", (p, 16, 16, 0, 4)),
        ("null pixels", (None, 16, 16, 6, 8)),
        ("host pixels", (on_host.ctypes.data, 16, 16, 6, 8)),
        ("pixels leave their allocation", (p, 16384, 16384, 6, 16)),
        ("2^32 pixels", (p, 65536, 65536, 0, 8)),
    ]
    rgb8 = {"colortype": 2, "bitdepth": 8, "palette": None, "key": None}
    pal = np.array([(0, 0, 0, 0)] * 5, dtype=np.uint8)
    for what, image in bad_images:
        im = api.PngImage(*image)
        stats = api.PngColorStats()
        ctypes.memset(ctypes.byref(stats), 0x5A, ctypes.sizeof(stats))
        assert fs(ctx.handle, ctypes.byref(im), ctypes.byref(stats)) != 0, what
        assert lib.zmx_last_error_class() == ZMX_ERR_REFUSED, (what, lib.zmx_last_error())
        assert bytes(stats) == b"\x5a" * ctypes.sizeof(stats), what
        assert fc(ctx.handle, ctypes.byref(im), ctypes.byref(mode_struct(rgb8)), q, d_out.numel()) != 0, what
        assert lib.zmx_last_error_class() == ZMX_ERR_REFUSED, (what, lib.zmx_last_error())
    assert b"2^32" in lib.zmx_last_error()
    good = api.PngImage(p, 16, 16, 6, 8)
    bad_converts = [
        ("colour type 1", {"colortype": 1, "bitdepth": 8, "palette": None, "key": None}, q, 4096),
        ("palette at 16 bits", {"colortype": 3, "bitdepth": 16, "palette": pal, "key": None}, q, 4096),
        ("RGB at 4 bits", {"colortype": 2, "bitdepth": 4, "palette": None, "key": None}, q, 4096),
        ("grey at 3 bits", {"colortype": 0, "bitdepth": 3, "palette": None, "key": None}, q, 4096),
        ("no palette", {"colortype": 3, "bitdepth": 8, "palette": pal[:0], "key": None}, q, 4096),
        ("5 entries at 2 bits", {"colortype": 3, "bitdepth": 2, "palette": pal, "key": None}, q, 4096),
        ("16 bits from 8", {"colortype": 2, "bitdepth": 16, "palette": None, "key": None}, q, 4096),
        ("capacity", rgb8, q, 16 * 16 * 3 - 1),
        ("null output", rgb8, None, 4096),
        ("host output", rgb8, on_host.ctypes.data, 4096),
        ("output overlaps the image", rgb8, p + 100, 4096),
    ]
    for what, mode, out, capacity in bad_converts:
        assert fc(ctx.handle, ctypes.byref(good), ctypes.byref(mode_struct(mode)), out, capacity) != 0, what
        assert lib.zmx_last_error_class() == ZMX_ERR_REFUSED, (what, lib.zmx_last_error())
    assert fc(ctx.handle, ctypes.byref(good), None, q, 4096) != 0 and lib.zmx_last_error_class() == ZMX_ERR_REFUSED
    assert fs(ctx.handle, ctypes.byref(good), None) != 0 and lib.zmx_last_error_class() == ZMX_ERR_REFUSED
    assert fs(None, ctypes.byref(good), ctypes.byref(api.PngColorStats())) != 0
    torch.cuda.synchronize()
    assert bool(torch.all(d_out == 0xA5)) and bool(torch.all(d_img == 0)) and not on_host.any(), "a refused call wrote"
    # and the valid call next to them works
    assert fc(ctx.handle, ctypes.byref(good), ctypes.byref(mode_struct(rgb8)), q, 16 * 16 * 3) == 0
    torch.cuda.synchronize()
    assert bool(torch.all(d_out[:16 * 16 * 3] == 0)) and bool(torch.all(d_out[16 * 16 * 3:] == 0xA5))
