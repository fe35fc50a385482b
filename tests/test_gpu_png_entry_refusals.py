"""What the device PNG entries say when they refuse a call: one table, a row per (entry, broken rule), the full text of
zmx_last_error() written out.  Every call breaks exactly one rule, so the text does not depend on the order of the checks.
The images are 4 x 3 and every call is refused before anything is compressed; in a batch the fault sits in image 1 of 3,
which pins the ": image 1" and ": range 1" infixes."""
import ctypes

import pytest
import torch

from zopfli_amd import ZopfliOptions, api

pytestmark = pytest.mark.gpu

ZMX_ERR_REFUSED = 3
PREDEFINED = 8
_size_p = ctypes.POINTER(ctypes.c_size_t)

# (entry, image kind, output shape, whether it takes lossy flags)
ENTRIES = [
    ("zmx_png_encode_device", "colour", "host", False),
    ("zmx_png_encode_device_lossy", "colour", "host", True),
    ("zmx_png_encode_device_to_device", "colour", "device", True),
    ("zmx_png_encode_device_batch", "colour", "batch", False),
    ("zmx_png_encode_device_batch_lossy", "colour", "batch", True),
    ("zmx_png_encode_device_batch_packed", "colour", "packed", True),
    ("zmx_png_optimize_device", "colour", "host", False),
    ("zmx_png_optimize_device_lossy", "colour", "host", True),
    ("zmx_png_optimize_device_to_device", "colour", "device", True),
    ("zmx_png_optimize_device_batch", "colour", "batch", False),
    ("zmx_png_optimize_device_batch_lossy", "colour", "batch", True),
    ("zmx_png_index_encode_device", "index", "host", True),
    ("zmx_png_index_optimize_device", "index", "host", True),
    ("zmx_png_index_encode_device_to_device", "index", "device", True),
    ("zmx_png_index_optimize_device_to_device", "index", "device", True),
    ("zmx_png_index_encode_device_batch", "index", "batch", True),
    ("zmx_png_index_optimize_device_batch", "index", "batch", True),
]

NOT_TAKEN = {"colour": "colour type 3 at 8 bits is not taken (0, 2, 4, 6 at 8 or 16)",
             "index": "colour type 2 at 8 bits is no index image (3 at 1, 2, 4, 8; 0 at 1, 2, 4)"}

# (rule, the output shapes it applies to, what is changed in a good call, the text behind "<entry>: ";
#  {image} is "" in a single call and "image 1: " in a batch, {range} likewise "range 1: ", {kind}: NOT_TAKEN's)
RULES = [
    ("width 0", "all", dict(image=dict(width=0)), "{image}width or height 0"),
    ("colour type", "all", dict(image=dict(colortype="other")), "{image}{kind}"),
    ("palette size", "index", dict(image=dict(bitdepth=2, palettesize=5)), "{image}a palette of 5 entries at 2 bits"),
    ("lossy 4", "lossy", dict(lossy=4), "unknown lossy flags 4"),
    ("strategy 9", "all", dict(strategy=9), "unknown strategy 9"),
    ("predefined in a batch", "many", dict(strategy=PREDEFINED), "ZMX_PNG_FILTER_PREDEFINED is the single call's"),
    ("predefined without types", "single", dict(strategy=PREDEFINED), "ZMX_PNG_FILTER_PREDEFINED without types"),
    ("predefined type 5", "single", dict(strategy=PREDEFINED, types=bytes([0, 1, 5])), "predefined type 5 of row 2"),
    ("null pixels", "all", dict(image=dict(d_pixels=None)), "{range}null pointer with a non-zero size"),
    ("d_out null", "to device", dict(dest="null"), "d_out: null pointer with a non-zero size"),
    ("d_out overlaps", "device", dict(dest="overlap"), "d_out overlaps image 0"),
    ("arena overlaps", "packed", dict(dest="overlap"), "d_out overlaps image 1"),
    ("align 3", "packed", dict(align=3), "align 3 is not a power of two from 1 to 4096"),
]


def _applies(where, kind, shape, lossy):
    return {"all": True, "index": kind == "index", "lossy": lossy, "many": shape in ("batch", "packed"),
            "single": shape in ("host", "device"), "to device": shape in ("device", "packed"), "device": shape == "device",
            "packed": shape == "packed"}[where]


def _image(kind, ptr, change):
    """A good 4 x 3 image at `ptr` — RGBA8, or indices at 8 bits with four colours — with `change` applied."""
    if kind == "colour":
        im = api.PngImage(ptr, 4, 3, 6, 8)
    else:
        im = api.PngIndexImage(ptr, 4, 3, 3, 8, 4)
        for k, rgba in enumerate([(0, 0, 0, 255), (255, 0, 0, 255), (0, 255, 0, 255), (0, 0, 255, 128)]):
            im.palette[4 * k:4 * k + 4] = rgba
    for field, value in (change or {}).items():
        if field == "colortype":
            value = 3 if kind == "colour" else 2
        setattr(im, field, value)
    return im


def _call(lib, entry, kind, shape, lossy_arg, base, change):
    """The entry on good arguments with `change` applied; images at base + 0, 256, 512, the destination at base + 2048."""
    struct = api.PngImage if kind == "colour" else api.PngIndexImage
    many = shape in ("batch", "packed")
    strategy, lossy, align = change.get("strategy", 6), change.get("lossy", 0), change.get("align", 1)
    dest = {"null": (None, 1024), "overlap": (base + (256 if many else 0), 64)}.get(change.get("dest"), (base + 2048, 1024))
    opts = ZopfliOptions(2)
    fn = getattr(lib, entry)
    fn.restype = ctypes.c_int
    if many:
        ims = (struct * 3)(*[_image(kind, base + 256 * i, change.get("image") if i == 1 else None) for i in range(3)])
        types, args = [ctypes.POINTER(ZopfliOptions), ctypes.c_size_t, ctypes.POINTER(struct), ctypes.c_int], [ctypes.byref(opts), 3, ims, strategy]
    else:
        im = _image(kind, base, change.get("image"))
        types = [ctypes.POINTER(ZopfliOptions), ctypes.POINTER(struct), ctypes.c_int, ctypes.c_char_p]
        args = [ctypes.byref(opts), ctypes.byref(im), strategy, change.get("types")]
    if lossy_arg:
        types, args = types + [ctypes.c_uint], args + [lossy]
    outsizes = (ctypes.c_size_t * 3)()
    if shape in ("host", "batch"):
        outs = (api._u8p * 3)()
        types, args = types + [ctypes.POINTER(api._u8p), _size_p], args + [outs, outsizes]
    elif shape == "device":
        types, args = types + [ctypes.c_void_p, ctypes.c_size_t, _size_p], args + [dest[0], dest[1], outsizes]
    else:
        offsets = (ctypes.c_size_t * 3)()
        types, args = types + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, _size_p, _size_p], args + [dest[0], dest[1], align, offsets, outsizes]
    fn.argtypes = types
    rc = fn(*args)
    nothing_out = all(int(s) == 0 for s in outsizes) and (shape not in ("host", "batch") or not any(bool(o) for o in outs))
    return rc, nothing_out


def test_every_refusal_says_what_it_said(gpu_lib):
    lib = gpu_lib
    room = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    base = room.data_ptr()
    wrong, rows = [], 0
    for entry, kind, shape, lossy_arg in ENTRIES:
        many = shape in ("batch", "packed")
        for rule, where, change, text in RULES:
            if not _applies(where, kind, shape, lossy_arg):
                continue
            rows += 1
            want = entry + ": " + text.format(image="image 1: " if many else "", range="range 1: " if many else "", kind=NOT_TAKEN[kind])
            rc, nothing_out = _call(lib, entry, kind, shape, lossy_arg, base, change)
            got = (rc, lib.zmx_last_error_class(), (lib.zmx_last_error() or b"").decode(), nothing_out)
            print(entry, "|", rule, "|", got[2])
            if got != (-1, ZMX_ERR_REFUSED, want, True):
                wrong.append((entry, rule, got, want))
    assert not wrong, wrong
    assert rows == 125   # (the table's size: a rule that stops applying anywhere shows here)
    assert not room.cpu().numpy().any(), "a refused call wrote something"
