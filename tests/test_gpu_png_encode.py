"""zmx_png_encode_device and its batch: an image in device memory as the PNG file zopflipng writes for it.  For the ten
small shapes of tests/png_encode_cases.py and every strategy the file is held against the one put together in Python —
the numpy-filtered scanlines (tests/png_rows_cases.py) with the types of the host-image row searches, the library's
host ZopfliCompress(ZLIB) with its header byte set, zlib.crc32 — and against the file the all-reference zopflipng writes
(oracle/_ref/zopflipng_ref, where it was built).  numiterations 2 throughout."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import png_encode_cases as ec
from png_rows_cases import filter_rows
from zopfli_amd import Context, ZopfliOptions, api
from zopfli_amd._build import PNG_REF

pytestmark = pytest.mark.gpu

ZMX_ERR_REFUSED = 3
ITERATIONS = 2
STRATEGIES = list(range(8)) + [ec.PREDEFINED]


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    c = Context(0, gpu_lib)
    yield c
    c.close()


def _types(ctx, lib, img, bw, strategy):
    """The filter type of every row under `strategy`, from the entries that take the image from the host."""
    h, n = img.shape
    if strategy <= 4:
        return np.full(h, strategy, dtype=np.uint8)
    if strategy == ec.PREDEFINED:
        return ec.mixed_types(h)
    out = np.zeros(h, dtype=np.uint8)
    if strategy == 7:
        fn = lib.zmx_png_filter_types_brute
        fn.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, ctypes.c_void_p]
        assert fn(ctx.handle, img.tobytes(), n, h, bw, 32768, out.ctypes.data) == 0, ctx.error()
        return out
    fn = lib.zmx_png_filter_types
    fn.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    assert fn(ctx.handle, img.tobytes(), n, h, bw, out.ctypes.data if strategy == 5 else None,
              out.ctypes.data if strategy == 6 else None) == 0, ctx.error()
    return out


def _expected(ctx, lib, shape, img, strategy):
    scan = filter_rows(img, ec.bytewidth(shape), _types(ctx, lib, img, ec.bytewidth(shape), strategy))
    stream = api.compress(scan.tobytes(), api.FORMAT_ZLIB, ZopfliOptions(ITERATIONS), lib=lib)
    return ec.assemble(shape, stream)


def _reference(tmp_path, shape, img, strategy):
    """The all-reference zopflipng's file, or None where it was not built."""
    if not os.path.exists(PNG_REF):
        return None
    src, dst = str(tmp_path / "in.png"), str(tmp_path / "ref.png")
    letter = "p" if strategy == ec.PREDEFINED else ec.STRATEGY_LETTERS[strategy]
    # (the input carries the types that --filters=p takes over)
    with open(src, "wb") as f:
        f.write(ec.plain_png(shape, filter_rows(img, ec.bytewidth(shape), ec.mixed_types(shape[1]))))
    r = subprocess.run([PNG_REF, "-y", "--always_zopflify", "--keepcolortype", f"--iterations={ITERATIONS}", f"--filters={letter}",
                        src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-1000:])
    with open(dst, "rb") as f:
        return f.read()


def _encode(lib, shape, d_img, strategy):
    predefined = ec.mixed_types(shape[1]) if strategy == ec.PREDEFINED else None
    return api.png_encode_device((d_img.data_ptr(),) + tuple(shape), strategy, ZopfliOptions(ITERATIONS), predefined=predefined, lib=lib)


@pytest.mark.parametrize("shape", ec.SHAPES, ids=ec.shape_id)
def test_encode(ctx, gpu_lib, tmp_path, shape):
    img = ec.pixels(shape)
    d_img = torch.from_numpy(img).cuda()
    torch.cuda.synchronize()
    for strategy in STRATEGIES:
        png = _encode(gpu_lib, shape, d_img, strategy)
        assert api.last_input_traffic(gpu_lib)[0] == 0, "pixels went host to device"
        assert [t for t, _ in ec.chunks(png)] == [b"IHDR", b"IDAT", b"IEND"]
        assert png == _expected(ctx, gpu_lib, shape, img, strategy), (shape, strategy)
        ref = _reference(tmp_path, shape, img, strategy)
        assert ref is None or png == ref, (shape, strategy, "zopflipng_ref")
    assert np.array_equal(d_img.cpu().numpy(), img), "the image changed"


def test_encode_wide_brute(ctx, gpu_lib, tmp_path):
    """Rows of 2400 bytes: the search's window of 32768 reaches where LodePNG's default of 2048 does not."""
    shape = ec.WIDE
    img = ec.pixels(shape)
    d_img = torch.from_numpy(img).cuda()
    torch.cuda.synchronize()
    png = _encode(gpu_lib, shape, d_img, 7)
    assert png == _expected(ctx, gpu_lib, shape, img, 7)
    ref = _reference(tmp_path, shape, img, 7)
    assert ref is None or png == ref


def test_batch_equals_singles(gpu_lib):
    shapes = ec.SHAPES + [ec.WIDE]
    imgs = [torch.from_numpy(ec.pixels(s)).cuda() for s in shapes]
    torch.cuda.synchronize()
    for strategy in (6, 7):
        singles = [_encode(gpu_lib, s, d, strategy) for s, d in zip(shapes, imgs)]
        images = [(d.data_ptr(),) + tuple(s) for s, d in zip(shapes, imgs)]
        assert api.png_encode_device_batch(images, strategy, ZopfliOptions(ITERATIONS), lib=gpu_lib) == singles
        assert api.last_input_traffic(gpu_lib)[0] == 0
        order = [7, 3, 10, 0, 9, 1, 8, 2, 6, 4, 5]
        got = api.png_encode_device_batch([images[i] for i in order], strategy, ZopfliOptions(ITERATIONS), lib=gpu_lib)
        assert got == [singles[i] for i in order]
    assert api.png_encode_device_batch([], "e", lib=gpu_lib) == []


def test_tensor_and_pointer_forms_agree(gpu_lib):
    rng = np.random.default_rng(9)
    for channels, colortype in ((None, 0), (2, 4), (3, 2), (4, 6)):
        hw = (13, 21) if channels is None else (13, 21, channels)
        t = torch.from_numpy(rng.integers(0, 40, size=hw, dtype=np.uint8)).cuda()
        a = api.png_encode_device(t, "m", ZopfliOptions(ITERATIONS), lib=gpu_lib)
        b = api.png_encode_device((t.data_ptr(), 21, 13, colortype, 8), 5, ZopfliOptions(ITERATIONS), lib=gpu_lib)
        assert a == b and ec.chunks(a)[0][1][8:10] == bytes([8, colortype])
        assert api.png_encode_device_batch([t, t], "m", ZopfliOptions(ITERATIONS), lib=gpu_lib) == [a, a]
    with pytest.raises(ValueError):
        api.png_encode_device(t[:, ::2], lib=gpu_lib)
    with pytest.raises(ValueError):
        api.png_encode_device(torch.zeros((4, 4, 5), dtype=torch.uint8, device="cuda:0"), lib=gpu_lib)
    with pytest.raises(ValueError):
        api.png_encode_device(torch.zeros((4, 4), dtype=torch.int16, device="cuda:0"), lib=gpu_lib)


def test_refusals_leave_out_untouched(gpu_lib):
    """ZMX_ERR_REFUSED before anything runs; (*out, *outsize) as they were."""
    lib = gpu_lib
    d_img = torch.zeros(64 * 64 * 8, dtype=torch.uint8, device="cuda:0")
    on_host = np.zeros(4096, dtype=np.uint8)
    torch.cuda.synchronize()
    p = d_img.data_ptr()
    fn = lib.zmx_png_encode_device
    fn.argtypes = [ctypes.POINTER(ZopfliOptions), ctypes.POINTER(api.PngImage), ctypes.c_int, ctypes.c_char_p,
                   ctypes.POINTER(api._u8p), ctypes.POINTER(ctypes.c_size_t)]
    fn.restype = ctypes.c_int
    fb = lib.zmx_png_encode_device_batch
    fb.argtypes = [ctypes.POINTER(ZopfliOptions), ctypes.c_size_t, ctypes.POINTER(api.PngImage), ctypes.c_int,
                   ctypes.POINTER(api._u8p), ctypes.POINTER(ctypes.c_size_t)]
    fb.restype = ctypes.c_int
    opts = ZopfliOptions(ITERATIONS)
    refused = [
        ("width 0", (p, 0, 16, 6, 8), 6, None),
        ("height 0", (p, 16, 0, 6, 8), 6, None),
        ("palette", (p, 16, 16, 3, 8), 6, None),
        ("colour type 1", (p, 16, 16, 1, 8), 6, None),
        ("depth 4", (p, 16, 16, 0, 4), 6, None),
        ("depth 32", (p, 16, 16, 0, 32), 6, None),
        ("strategy 9", (p, 16, 16, 6, 8), 9, None),
        ("strategy -1", (p, 16, 16, 6, 8), -1, None),
        ("predefined without types", (p, 16, 16, 6, 8), 8, None),
        ("predefined type 5", (p, 16, 16, 6, 8), 8, bytes([0] * 15 + [5])),
        ("null pixels", (None, 16, 16, 6, 8), 6, None),
        ("host pixels", (on_host.ctypes.data, 16, 16, 6, 8), 6, None),
        ("pixels leave their allocation", (p, 16384, 16384, 6, 16), 6, None),      # 2 GiB from a tensor of 32 KiB
    ]
    sentinel = api._libc.malloc(8)
    ctypes.memmove(sentinel, b"abc", 3)
    try:
        for what, image, strategy, types in refused:
            out, size = ctypes.cast(sentinel, api._u8p), ctypes.c_size_t(3)
            im = api.PngImage(*image)
            assert fn(ctypes.byref(opts), ctypes.byref(im), strategy, types, ctypes.byref(out), ctypes.byref(size)) != 0, what
            assert lib.zmx_last_error_class() == ZMX_ERR_REFUSED, (what, lib.zmx_last_error())
            assert ctypes.cast(out, ctypes.c_void_p).value == sentinel and size.value == 3, what
            # the same image in the middle of a batch: no out[i] changes
            good = api.PngImage(p, 16, 16, 6, 8)
            arr = (api.PngImage * 3)(good, im, good)
            outs = (api._u8p * 3)(*[ctypes.cast(sentinel, api._u8p)] * 3)
            sizes = (ctypes.c_size_t * 3)(3, 3, 3)
            assert fb(ctypes.byref(opts), 3, arr, strategy, outs, sizes) != 0, what
            assert lib.zmx_last_error_class() == ZMX_ERR_REFUSED, (what, lib.zmx_last_error())
            assert all(ctypes.cast(outs[i], ctypes.c_void_p).value == sentinel and sizes[i] == 3 for i in range(3)), what
        assert ctypes.string_at(sentinel, 3) == b"abc"
        # the batch refuses predefined types whatever the images
        arr = (api.PngImage * 1)(api.PngImage(p, 16, 16, 6, 8))
        outs, sizes = (api._u8p * 1)(), (ctypes.c_size_t * 1)(0)
        assert fb(ctypes.byref(opts), 1, arr, 8, outs, sizes) != 0 and lib.zmx_last_error_class() == ZMX_ERR_REFUSED
        assert not outs[0] and sizes[0] == 0
    finally:
        api._libc.free(sentinel)
    # and the next valid call appends to what it is given
    out, size = api._u8p(), ctypes.c_size_t(0)
    im = api.PngImage(p, 16, 16, 6, 8)
    assert fn(ctypes.byref(opts), ctypes.byref(im), 6, None, ctypes.byref(out), ctypes.byref(size)) == 0
    first = ctypes.string_at(out, size.value)
    assert fn(ctypes.byref(opts), ctypes.byref(im), 6, None, ctypes.byref(out), ctypes.byref(size)) == 0
    assert ctypes.string_at(out, size.value) == first + first
    api._libc.free(out)
