"""Palette, 1/2/4-bit grey and index images in device memory: the zmx_png_index_* entries on every case of
tests/png_index_cases.py.  The two kernels are held word for word against the numpy model, source and destination at odd
addresses, guard bytes around the output.  The optimize entry's file is png_optimize_device's file of the RGBA8 expansion;
the encode entry's is put together in Python from the model's rows, the host-image row searches, the library's
ZopfliCompress(ZLIB) and png_color_cases' container.  Both are the all-reference zopflipng's where it was built, and always
tests/golden/png_index.json's.  The _out forms, the batches, the refusals.  numiterations 2."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import png_color_cases as cc
import png_index_cases as ic
from png_rows_cases import filter_rows
from zopfli_amd import Context, ZopfliOptions, api
from zopfli_amd._build import PNG_REF, ROOT

pytestmark = pytest.mark.gpu

ZMX_ERR_REFUSED = 3
ITERATIONS = 2
STRATEGIES = list(range(8)) + ["auto"]
LETTERS = {0: "0", 1: "1", 2: "2", 3: "3", 4: "4", 5: "m", 6: "e", 7: "b", "auto": "auto"}
GUARD = 64
FILL = 0xa5
SMALL_NAMES = [c[0] for c in ic.CASES if c[1] * c[2] <= 1000]


def _opts():
    return ZopfliOptions(ITERATIONS)


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    c = Context(0, gpu_lib)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "png_index.json")) as f:
        return json.load(f)["files"]


def _upload(arr, offset=0):
    """The bytes on the device, `offset` bytes behind a 256-byte boundary: (the tensor that owns them, the pointer)."""
    flat = np.ascontiguousarray(arr, dtype=np.uint8).reshape(-1)
    d = torch.zeros(offset + flat.size, dtype=torch.uint8, device="cuda:0")
    d[offset:] = torch.from_numpy(flat.copy()).cuda()
    torch.cuda.synchronize()
    assert d.data_ptr() % 256 == 0
    return d, d.data_ptr() + offset


def _image(case, ptr):
    name, w, h, ct, depth, pal = case
    return (ptr, w, h, ct, depth, None if ct != 3 else ic.palette_of(case))


def _mode(m):
    """png_color_cases' mode as a PngColorMode."""
    out = api.PngColorMode()
    out.colortype, out.bitdepth = m["colortype"], m["bitdepth"]
    if m["palette"] is not None:
        pal = np.ascontiguousarray(m["palette"], dtype=np.uint8)
        out.palettesize = len(pal)
        for i, b in enumerate(pal.reshape(-1)):
            out.palette[i] = int(b)
    if m["key"] is not None:
        out.key_defined = 1
        out.key_r, out.key_g, out.key_b = m["key"]
    return out


def _modes(case, lossy):
    _, w, h, _, _, _ = case
    st = cc.stats(ic.expand(case, lossy), 8)
    return st, ic.keep_mode(case, lossy), cc.choose(st, w * h), cc.retry_mode(st, w * h)


@pytest.mark.parametrize("case", ic.CASES, ids=ic.IDS)
def test_kernels(ctx, gpu_lib, case):
    name, w, h, ct, depth, _ = case
    offset = 1 + sum(name.encode()) % 15
    d_img, ptr = _upload(ic.packed(case), offset)
    image = _image(case, ptr)
    first = ctx.png_index_use_device(image)
    assert first == ic.first_table(ic.values(case)), name
    assert ctx.png_index_use_device(image) == first, "the table differs from run to run"
    for lossy in (0, 1):
        st, keep, chosen, retry = _modes(case, lossy)
        got = api.png_index_color_stats(image, first, lossy_transparent=bool(lossy), lib=gpu_lib)
        assert (got.colored, got.key, got.alpha, got.numcolors, got.bits) == (int(st["colored"]), int(st["key"]), int(st["alpha"]), st["numcolors"], st["bits"])
        assert (got.key_r, got.key_g, got.key_b) == st["key_rgb"] and got.colors() == [tuple(int(x) for x in e) for e in st["palette"]]
        kmode, ktable = api.png_index_keep_plan(image, first, lossy_transparent=bool(lossy), lib=gpu_lib)
        assert (kmode.colortype, kmode.bitdepth) == (ct, depth)
        if ct == 3:
            assert kmode.colors() == [tuple(int(x) for x in e) for e in keep["palette"]], (name, lossy)
        for k, mode in enumerate((keep, chosen, retry)):
            table = ktable if k == 0 else api.png_index_table(image, first, _mode(mode), lossy_transparent=bool(lossy), lib=gpu_lib)
            want = ic.convert_table(ic.values(case), ic.table_for(ic.seen_palette(case, lossy), mode), mode)
            assert np.array_equal(want, cc.convert(ic.expand(case, lossy), 8, w, h, mode))
            to = (offset * 7 + 3 * k + lossy) % 16
            d_out = torch.full((GUARD + to + want.size + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            ctx.png_index_convert_device(image, _mode(mode), table, d_out.data_ptr() + GUARD + to, want.size)
            host = d_out.cpu().numpy()
            assert np.array_equal(host[GUARD + to:GUARD + to + want.size], want.reshape(-1)), (name, lossy, k)
            assert (host[:GUARD + to] == FILL).all() and (host[GUARD + to + want.size:] == FILL).all(), "a byte outside the output was written"
    assert np.array_equal(d_img.cpu().numpy()[offset:], ic.packed(case).reshape(-1)), "the image changed"


@pytest.mark.parametrize("case,at", ic.OUTSIDE, ids=[c[0][0] for c in ic.OUTSIDE])
def test_value_outside_the_palette(ctx, gpu_lib, case, at):
    name, w, h, ct, depth, _ = case
    d_img, ptr = _upload(ic.packed(case), 5)
    image = _image(case, ptr)
    first = ctx.png_index_use_device(image)
    assert first == ic.first_table(ic.values(case))
    mode = api.PngColorMode()
    mode.colortype, mode.bitdepth, mode.palettesize = 3, depth, len(ic.palette_of(case))
    d_out = torch.zeros(h * w + 16, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(RuntimeError, match=f"pixel {at} "):
        ctx.png_index_convert_device(image, mode, list(range(256)), d_out)
    assert gpu_lib.zmx_last_error_class() == ZMX_ERR_REFUSED
    for entry in (api.png_index_encode_device, api.png_index_optimize_device):
        with pytest.raises(RuntimeError, match=f"pixel {at} "):
            entry(image, 0, _opts(), lib=gpu_lib)
        assert gpu_lib.zmx_last_error_class() == ZMX_ERR_REFUSED
    with pytest.raises(RuntimeError, match=f"pixel {at} "):
        api.png_index_color_stats(image, first, lib=gpu_lib)


def _reference(tmp_path, case, strategy, keep, lossy):
    """The all-reference zopflipng's file for the case as a palette or low-bit grey PNG, or None where it was not built."""
    if not os.path.exists(PNG_REF):
        return None
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_png_index_golden as mk
    return mk.reference(str(tmp_path), case, LETTERS[strategy], keep, lossy)


@pytest.mark.parametrize("case", ic.CASES, ids=ic.IDS)
def test_optimize_is_the_expansions_file(gpu_lib, golden, tmp_path, case):
    """Every strategy and "auto", with and without --lossy_transparent: byte for byte png_optimize_device of the RGBA8 tensor."""
    name, w, h, ct, depth, _ = case
    d_img, ptr = _upload(ic.packed(case), 3)
    d_rgba, rgba_ptr = _upload(ic.expand(case).astype(np.uint8))
    image, rgba = _image(case, ptr), (rgba_ptr, w, h, 6, 8)
    for lossy in (False, True):
        for strategy in STRATEGIES:
            png = api.png_index_optimize_device(image, strategy, _opts(), lib=gpu_lib, lossy_transparent=lossy)
            assert api.last_input_traffic(gpu_lib)[0] == 0, "indices went host to device"
            assert png == api.png_optimize_device(rgba, strategy, _opts(), lib=gpu_lib, lossy_transparent=lossy), (name, strategy, lossy)
            key = f"{name}|optimize|{LETTERS[strategy]}|{int(lossy)}"
            if key in golden:
                assert png.hex() == golden[key], key
            if strategy in (0, 6, "auto") and w * h <= 1000:
                ref = _reference(tmp_path, case, strategy, False, int(lossy))
                assert ref is None or png == ref, (name, strategy, lossy, "zopflipng_ref")
    assert np.array_equal(d_img.cpu().numpy()[3:], ic.packed(case).reshape(-1)), "the image changed"


def _types(ctx, lib, rows, bytewidth, strategy):
    """The filter types of the host-image row searches (zmx_png_filter_types, zmx_png_filter_types_brute)."""
    import ctypes
    h, n = rows.shape
    if strategy in range(5):
        return np.full(h, strategy, dtype=np.uint8)
    out = np.zeros(h, dtype=np.uint8)
    img = np.ascontiguousarray(rows)
    if strategy == 7:
        fn = lib.zmx_png_filter_types_brute
        fn.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, ctypes.c_void_p]
        assert fn(ctx.handle, img.tobytes(), n, h, bytewidth, 32768, out.ctypes.data) == 0, ctx.error()
        return out
    fn = lib.zmx_png_filter_types
    fn.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    assert fn(ctx.handle, img.tobytes(), n, h, bytewidth, out.ctypes.data if strategy == 5 else None,
              out.ctypes.data if strategy == 6 else None) == 0, ctx.error()
    return out


@pytest.mark.parametrize("case", ic.CASES, ids=ic.IDS)
def test_encode_is_the_assembled_file(ctx, gpu_lib, golden, tmp_path, case):
    """The --keepcolortype file: the model's rows in the input's mode (the palette whole, shrunk after the lossy rewrite),
    filtered with the types of the host-image row searches, ZopfliCompress(ZLIB) of the library, PLTE / tRNS by color_chunks."""
    name, w, h, ct, depth, _ = case
    d_img, ptr = _upload(ic.packed(case), 9)
    image = _image(case, ptr)
    for lossy in (0, 1):
        mode = ic.keep_mode(case, lossy)
        rows = ic.convert_table(ic.values(case), ic.table_for(ic.seen_palette(case, lossy), mode), mode)
        made = {}
        for strategy in range(8):
            png = api.png_index_encode_device(image, strategy, _opts(), lib=gpu_lib, lossy_transparent=bool(lossy))
            assert api.last_input_traffic(gpu_lib)[0] == 0, "indices went host to device"
            scan = filter_rows(rows, 1, _types(ctx, gpu_lib, rows, 1, strategy))
            assert png == cc.assemble(w, h, mode, api.compress(scan.tobytes(), api.FORMAT_ZLIB, _opts(), lib=gpu_lib)), (name, strategy, lossy)
            made[strategy] = png
            key = f"{name}|keep|{LETTERS[strategy]}|{lossy}"
            if key in golden:
                assert png.hex() == golden[key], key
            if strategy in (0, 6) and w * h <= 1000:
                ref = _reference(tmp_path, case, strategy, True, lossy)
                assert ref is None or png == ref, (name, strategy, lossy, "zopflipng_ref")
        chosen, sizes = ctx.png_index_choose_strategy_device(image, reduce_color=False, lossy_transparent=bool(lossy))
        auto = api.png_index_encode_device(image, "auto", _opts(), lib=gpu_lib, lossy_transparent=bool(lossy))
        assert chosen in range(7) and auto == made[chosen] and sizes[7] == 0 and min(sizes[:7]) == sizes[chosen], (name, lossy, chosen, sizes)
        key = f"{name}|keep|auto|{lossy}"
        if key in golden:
            assert auto.hex() == golden[key], key
        if w * h <= 1000:
            ref = _reference(tmp_path, case, "auto", True, lossy)
            assert ref is None or auto == ref, (name, lossy, "zopflipng_ref without --filters")
    assert np.array_equal(d_img.cpu().numpy()[9:], ic.packed(case).reshape(-1)), "the image changed"


def test_tensor_with_palette(gpu_lib):
    """A 2-D uint8 CUDA tensor of labels with palette= (n x 3: opaque) is the tuple form at 8 bits."""
    case = ic.case("last-pixel")
    name, w, h, ct, depth, _ = case
    labels = torch.from_numpy(ic.values(case).copy()).cuda()
    pal3 = ic.palette_of(case)[:, :3]
    for entry in (api.png_index_encode_device, api.png_index_optimize_device):
        assert entry(labels, "e", _opts(), lib=gpu_lib, palette=pal3) == entry((labels, w, h, 3, 8, ic.palette_of(case)), "e", _opts(), lib=gpu_lib)
    with pytest.raises(ValueError):
        api.png_index_encode_device(labels, "e", _opts(), lib=gpu_lib)


class Dest:
    """`capacity` bytes of device memory `offset` bytes behind a 256-byte boundary, 0xA5 all over, guards on both sides."""

    def __init__(self, capacity, offset=0):
        self.capacity, self.at = capacity, GUARD + offset
        self.buf = torch.full((GUARD + offset + capacity + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        assert self.buf.data_ptr() % 256 == 0

    @property
    def pair(self):
        return (self.buf.data_ptr() + self.at, self.capacity)

    def file(self, size):
        host = self.buf.cpu().numpy()
        assert (host[:self.at] == FILL).all() and (host[self.at + size:] == FILL).all(), "a byte outside the file was written"
        return host[self.at:self.at + size].tobytes()

    def untouched(self):
        return bool((self.buf.cpu().numpy() == FILL).all())


OUT_NAMES = ["b1-w17-h3", "b2-w1-h1", "two-equal", "unused", "grey-key", "few-rgba", "two-transparent", "last-pixel", "grey4-wide", "big1"]


@pytest.mark.parametrize("name", OUT_NAMES)
def test_out_forms_equal_the_host_output_files(gpu_lib, name):
    case = ic.case(name)
    _, w, h, ct, depth, _ = case
    d_img, ptr = _upload(ic.packed(case), 2)
    image = _image(case, ptr)
    bound = api.png_index_bound(w, h, ct, depth, lib=gpu_lib)
    for host, out in ((api.png_index_encode_device, api.png_index_encode_device_out), (api.png_index_optimize_device, api.png_index_optimize_device_out)):
        for lossy in (False, True):
            for strategy, offset in ((0, 0), (6, 1), ("auto", 7)):
                want = host(image, strategy, _opts(), lib=gpu_lib, lossy_transparent=lossy)
                assert bound >= len(want)
                dst = Dest(bound, offset)
                size = out(image, dst.pair, strategy, _opts(), lib=gpu_lib, lossy_transparent=lossy)
                assert api.last_input_traffic(gpu_lib)[0] == 0 and api.last_output_traffic(gpu_lib)[0] == 0, "a byte visited the host"
                assert size == len(want) and dst.file(size) == want, (name, strategy, lossy, offset)
    # exactly the file's size does; one byte less is refused with the size and nothing written
    want = api.png_index_optimize_device(image, 0, _opts(), lib=gpu_lib)
    dst = Dest(len(want), 1)
    assert api.png_index_optimize_device_out(image, dst.pair, 0, _opts(), lib=gpu_lib) == len(want) and dst.file(len(want)) == want
    dst = Dest(len(want) - 1, 1)
    with pytest.raises(api.CapacityError) as e:
        api.png_index_optimize_device_out(image, dst.pair, 0, _opts(), lib=gpu_lib)
    assert e.value.needed == len(want) and dst.untouched()
    assert np.array_equal(d_img.cpu().numpy()[2:], ic.packed(case).reshape(-1)), "the image changed"


def test_bound(gpu_lib):
    for w, h in ((1, 1), (17, 3), (600, 300), (4096, 4096)):
        assert api.png_index_bound(w, h, 3, 1, lib=gpu_lib) == api.png_bound(w, h, 6, 8, lib=gpu_lib) > 0
    for ct, depth in ((0, 8), (3, 16), (2, 8), (3, 3), (0, 0)):
        assert api.png_index_bound(8, 8, ct, depth, lib=gpu_lib) == 0
    assert api.png_index_bound(0, 8, 3, 8, lib=gpu_lib) == 0 and api.png_index_bound(1 << 16, 1 << 16, 3, 8, lib=gpu_lib) == 0


def test_batches_equal_singles(gpu_lib):
    names = SMALL_NAMES[::4] + ["two-equal", "unused", "grey-key-16px", "two-transparent", "big8"]
    held = [_upload(ic.packed(ic.case(n)), 1 + i % 15) for i, n in enumerate(names)]
    images = [_image(ic.case(n), ptr) for n, (_, ptr) in zip(names, held)]
    order = [(5 * i + 2) % len(images) for i in range(len(images))]
    assert sorted(order) == list(range(len(images)))
    for single, batch in ((api.png_index_encode_device, api.png_index_encode_device_batch),
                          (api.png_index_optimize_device, api.png_index_optimize_device_batch)):
        for strategy, lossy in ((0, False), (6, True), ("auto", True)):
            singles = [single(im, strategy, _opts(), lib=gpu_lib, lossy_transparent=lossy) for im in images]
            assert batch([images[i] for i in order], strategy, _opts(), lib=gpu_lib, lossy_transparent=lossy) == [singles[i] for i in order]
            assert api.last_input_traffic(gpu_lib)[0] == 0
        assert batch([], 0, _opts(), lib=gpu_lib) == []
    for n, (d, _), i in zip(names, held, range(len(names))):
        assert np.array_equal(d.cpu().numpy()[1 + i % 15:], ic.packed(ic.case(n)).reshape(-1)), "an image changed"


def test_refusals(ctx, gpu_lib):
    import ctypes
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    p = d.data_ptr()
    pal = ic.FOUR
    bad = [("width 0", (p, 0, 16, 3, 8, pal)), ("colour type 2", (p, 16, 16, 2, 8, pal)), ("grey at 8 bits", (p, 16, 16, 0, 8, None)),
           ("depth 3", (p, 16, 16, 3, 3, pal)), ("palettesize above 2^bitdepth", (p, 16, 16, 3, 1, pal)),
           ("2^32 pixels", (p, 1 << 16, 1 << 16, 3, 1, ic.BW)), ("null pixels", (0, 16, 16, 3, 8, pal)),
           ("pixels leave their allocation", (p, 4096, 4096, 3, 8, pal))]
    out, outsize = ctypes.POINTER(ctypes.c_ubyte)(), ctypes.c_size_t(0)
    for what, image in bad:
        im = api._png_index_image(image)
        for name in ("zmx_png_index_encode_device", "zmx_png_index_optimize_device"):
            fn = getattr(gpu_lib, name)
            fn.argtypes = [ctypes.POINTER(ZopfliOptions), ctypes.POINTER(api.PngIndexImage), ctypes.c_int, ctypes.c_char_p, ctypes.c_uint,
                           ctypes.POINTER(ctypes.POINTER(ctypes.c_ubyte)), ctypes.POINTER(ctypes.c_size_t)]
            fn.restype = ctypes.c_int
            assert fn(ctypes.byref(_opts()), ctypes.byref(im), 0, None, 0, ctypes.byref(out), ctypes.byref(outsize)) == -1, what
            assert gpu_lib.zmx_last_error_class() == ZMX_ERR_REFUSED and not out and outsize.value == 0, what
        with pytest.raises(RuntimeError, match="zmx_png_index_use_device"):
            ctx.png_index_use_device(image)
        with pytest.raises(RuntimeError):
            api.png_index_encode_device_batch([(p, 4, 4, 3, 8, pal), image], 0, _opts(), lib=gpu_lib)
    zero = api._png_index_image((p, 16, 16, 3, 8, pal))
    zero.palettesize = 0
    fn = gpu_lib.zmx_png_index_encode_device
    assert fn(ctypes.byref(_opts()), ctypes.byref(zero), 0, None, 0, ctypes.byref(out), ctypes.byref(outsize)) == -1 and outsize.value == 0
    good = (p, 16, 16, 3, 8, pal)
    for strategy, lossy, types in ((9, 0, None), (8, 0, None), (0, 4, None), (8, 0, bytes([5] * 16))):
        im = api._png_index_image(good)
        assert fn(ctypes.byref(_opts()), ctypes.byref(im), strategy, types, lossy, ctypes.byref(out), ctypes.byref(outsize)) == -1
        assert gpu_lib.zmx_last_error_class() == ZMX_ERR_REFUSED and not out and outsize.value == 0, (strategy, lossy)
    with pytest.raises(RuntimeError):
        api.png_index_encode_device_batch([good], 8, _opts(), lib=gpu_lib)
    # a mode outside the table, a capacity below the output's size, an output that overlaps the image
    mode = api.PngColorMode()
    mode.colortype, mode.bitdepth = 6, 16
    with pytest.raises(RuntimeError, match="no mode an index image converts to"):
        ctx.png_index_convert_device(good, mode, [0] * 256, torch.zeros(4096, dtype=torch.uint8, device="cuda:0"))
    mode.bitdepth = 8
    with pytest.raises(RuntimeError, match="capacity"):
        ctx.png_index_convert_device(good, mode, [0] * 256, torch.zeros(1023, dtype=torch.uint8, device="cuda:0"))
    with pytest.raises(RuntimeError, match="overlaps"):
        ctx.png_index_convert_device(good, mode, [0] * 256, p + 128, 1024)
    # the existing entries still refuse such input
    with pytest.raises(RuntimeError):
        api.png_encode_device((p, 16, 16, 3, 8), 0, _opts(), lib=gpu_lib)
    # a good image still goes through
    assert api.png_index_encode_device(good, 0, _opts(), lib=gpu_lib)[:8] == b"\x89PNG\r\n\x1a\n"
