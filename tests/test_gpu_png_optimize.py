"""zmx_png_optimize_device and its batch: an image in device memory as the PNG file zopflipng writes for it without
--keepcolortype.  For every case of tests/png_color_cases.py and the strategies 0 4 m e b (p on three cases) the file is
held against the one put together in Python — the model's mode and converted image, the numpy-filtered scanlines
(tests/png_rows_cases.py) with the types of the host-image row searches, the library's host ZopfliCompress(ZLIB), the
container of png_color_cases.assemble, the second try where the palette file is below 4096 bytes — and against the file
the all-reference zopflipng writes (oracle/_ref/zopflipng_ref, where it was built).  numiterations 2 throughout."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import png_color_cases as cc
import png_encode_cases as ec
from png_rows_cases import filter_rows
from zopfli_amd import Context, ZopfliOptions, api
from zopfli_amd._build import PNG_REF

pytestmark = pytest.mark.gpu

ZMX_ERR_REFUSED = 3
ITERATIONS = 2
STRATEGIES = [0, 4, 5, 6, 7]
PREDEFINED_CASES = ["colors-5", "grey2-w37-ct6", "key"]


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


def _file_in(ctx, lib, case, mode, strategy):
    name, w, h, ct, depth = case
    conv = np.ascontiguousarray(cc.convert(cc.model(case)[0], depth, w, h, mode))
    scan = filter_rows(conv, cc.bytewidth(mode), _types(ctx, lib, conv, cc.bytewidth(mode), strategy))
    return cc.assemble(w, h, mode, api.compress(scan.tobytes(), api.FORMAT_ZLIB, ZopfliOptions(ITERATIONS), lib=lib))


def _expected(ctx, lib, case, strategy):
    """(file, its mode, whether the second try replaced the first: None where none is made)."""
    name, w, h, ct, depth = case
    rgba, st, mode, conv = cc.model(case)
    first = _file_in(ctx, lib, case, mode, strategy)
    if mode["colortype"] != 3 or len(first) >= cc.RETRY_BELOW:
        return first, mode, None
    again = cc.retry_mode(st, w * h)
    second = _file_in(ctx, lib, case, again, strategy)
    return (second, again, True) if len(second) < len(first) else (first, mode, False)


def _reference(tmp_path, case, strategy):
    """The all-reference zopflipng's file, or None where it was not built."""
    if not os.path.exists(PNG_REF):
        return None
    name, w, h, ct, depth = case
    src, dst = str(tmp_path / "in.png"), str(tmp_path / "ref.png")
    letter = "p" if strategy == ec.PREDEFINED else ec.STRATEGY_LETTERS[strategy]
    # (the input carries the types that --filters=p takes over)
    with open(src, "wb") as f:
        f.write(ec.plain_png((w, h, ct, depth), filter_rows(cc.pixels(case), ec.CHANNELS[ct] * depth // 8, ec.mixed_types(h))))
    r = subprocess.run([PNG_REF, "-y", "--always_zopflify", f"--iterations={ITERATIONS}", f"--filters={letter}", src, dst],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-1000:])
    with open(dst, "rb") as f:
        return f.read()


def _optimize(lib, case, d_img, strategy):
    name, w, h, ct, depth = case
    predefined = ec.mixed_types(h) if strategy == ec.PREDEFINED else None
    return api.png_optimize_device((d_img.data_ptr(), w, h, ct, depth), strategy, ZopfliOptions(ITERATIONS), predefined=predefined, lib=lib)


def _on_device(case):
    d_img = torch.from_numpy(cc.pixels(case).copy()).cuda()
    torch.cuda.synchronize()
    return d_img


@pytest.mark.parametrize("case", cc.CASES, ids=cc.IDS)
def test_optimize(ctx, gpu_lib, tmp_path, case):
    name, w, h, ct, depth = case
    d_img = _on_device(case)
    for strategy in STRATEGIES + ([ec.PREDEFINED] if name in PREDEFINED_CASES else []):
        png = _optimize(gpu_lib, case, d_img, strategy)
        assert api.last_input_traffic(gpu_lib)[0] == 0, "pixels went host to device"
        want, mode, retried = _expected(ctx, gpu_lib, case, strategy)
        assert [t for t, _ in ec.chunks(png)] == cc.expected_chunks(mode), (name, strategy)
        assert png == want, (name, strategy)
        ref = _reference(tmp_path, case, strategy)
        assert ref is None or png == ref, (name, strategy, "zopflipng_ref")
        if strategy == 0:
            assert retried == cc.EXPECT[name][4], (name, "the second try")
        if name in cc.AS_IS:
            predefined = ec.mixed_types(h) if strategy == ec.PREDEFINED else None
            assert png == api.png_encode_device((d_img.data_ptr(), w, h, ct, depth), strategy, ZopfliOptions(ITERATIONS),
                                                predefined=predefined, lib=gpu_lib), (name, strategy, "png_encode_device")
    assert np.array_equal(d_img.cpu().numpy(), cc.pixels(case)), "the image changed"


BATCH = ["colors-1", "colors-17", "colors-256", "colors-alpha-only", "key", "grey-key", "grey1-w9-ct6", "grey4-w37-ct0", "fake16",
         "fake16-ga", "true16-rgb-key", "true16-rgba", "exactly-2n", "retry-40", "retry-100-alpha", "unchanged", "colors-257"]


def test_batch_equals_singles(gpu_lib):
    cases = [cc.CASES[cc.IDS.index(n)] for n in BATCH]
    imgs = [_on_device(c) for c in cases]
    images = [(d.data_ptr(),) + tuple(c[1:]) for c, d in zip(cases, imgs)]
    for strategy in (0, 6):
        singles = [_optimize(gpu_lib, c, d, strategy) for c, d in zip(cases, imgs)]
        # (both kinds of second try are in: one that wins and one that loses)
        kinds = [ec.chunks(s)[0][1][9] for s in singles]
        assert kinds[BATCH.index("retry-40")] == 2 and kinds[BATCH.index("retry-100-alpha")] == 3
        assert api.png_optimize_device_batch(images, strategy, ZopfliOptions(ITERATIONS), lib=gpu_lib) == singles
        assert api.last_input_traffic(gpu_lib)[0] == 0
        order = [(7 * i + 3) % len(cases) for i in range(len(cases))]
        assert sorted(order) == list(range(len(cases)))
        got = api.png_optimize_device_batch([images[i] for i in order], strategy, ZopfliOptions(ITERATIONS), lib=gpu_lib)
        assert got == [singles[i] for i in order]
    assert api.png_optimize_device_batch([], "e", lib=gpu_lib) == []
    # a batch without any second try
    plain = [images[BATCH.index(n)] for n in ("unchanged", "key")]
    assert api.png_optimize_device_batch(plain, 6, ZopfliOptions(ITERATIONS), lib=gpu_lib) == \
        [_optimize(gpu_lib, cases[BATCH.index(n)], imgs[BATCH.index(n)], 6) for n in ("unchanged", "key")]


def test_tensor_form(gpu_lib):
    """A uint8 tensor (H, W, 4) whose alpha is all 255 and whose channels are equal ends as grey."""
    g = torch.arange(13 * 21, dtype=torch.int64).reshape(13, 21).remainder(251).to(torch.uint8)
    t = torch.stack([g, g, g, torch.full_like(g, 255)], dim=2).contiguous().cuda()
    a = api.png_optimize_device(t, "m", ZopfliOptions(ITERATIONS), lib=gpu_lib)
    assert ec.chunks(a)[0][1][8:10] == bytes([8, 0])
    assert a == api.png_encode_device(g.cuda(), "m", ZopfliOptions(ITERATIONS), lib=gpu_lib)
    assert api.png_optimize_device_batch([t, t], "m", ZopfliOptions(ITERATIONS), lib=gpu_lib) == [a, a]


def test_refusals_leave_out_untouched(gpu_lib):
    """ZMX_ERR_REFUSED before anything runs; (*out, *outsize) as they were, in the batch every one of them."""
    lib = gpu_lib
    d_img = torch.zeros(64 * 64 * 8, dtype=torch.uint8, device="cuda:0")
    on_host = np.zeros(4096, dtype=np.uint8)
    torch.cuda.synchronize()
    p = d_img.data_ptr()
    fn = lib.zmx_png_optimize_device
    fn.argtypes = [ctypes.POINTER(ZopfliOptions), ctypes.POINTER(api.PngImage), ctypes.c_int, ctypes.c_char_p,
                   ctypes.POINTER(api._u8p), ctypes.POINTER(ctypes.c_size_t)]
    fn.restype = ctypes.c_int
    fb = lib.zmx_png_optimize_device_batch
    fb.argtypes = [ctypes.POINTER(ZopfliOptions), ctypes.c_size_t, ctypes.POINTER(api.PngImage), ctypes.c_int,
                   ctypes.POINTER(api._u8p), ctypes.POINTER(ctypes.c_size_t)]
    fb.restype = ctypes.c_int
    opts = ZopfliOptions(ITERATIONS)
    refused = [
        ("width 0", (p, 0, 16, 6, 8), 6, None),
        ("height 0", (p, 16, 0, 6, 8), 6, None),
        ("palette input", (p, 16, 16, 3, 8), 6, None),
        ("colour type 1", (p, 16, 16, 1, 8), 6, None),
        ("depth 4", (p, 16, 16, 0, 4), 6, None),
        ("depth 32", (p, 16, 16, 0, 32), 6, None),
        ("strategy 9", (p, 16, 16, 6, 8), 9, None),
        ("strategy -1", (p, 16, 16, 6, 8), -1, None),
        ("predefined without types", (p, 16, 16, 6, 8), 8, None),
        ("predefined type 5", (p, 16, 16, 6, 8), 8, bytes([0] * 15 + [5])),
        ("null pixels", (None, 16, 16, 6, 8), 6, None),
        ("host pixels", (on_host.ctypes.data, 16, 16, 6, 8), 6, None),
        ("pixels leave their allocation", (p, 16384, 16384, 6, 16), 6, None),
        ("2^32 pixels", (p, 65536, 65536, 0, 8), 6, None),
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
    # and the next valid call appends to what it is given (a flat image: the second try's file)
    out, size = api._u8p(), ctypes.c_size_t(0)
    im = api.PngImage(p, 16, 16, 6, 8)
    assert fn(ctypes.byref(opts), ctypes.byref(im), 6, None, ctypes.byref(out), ctypes.byref(size)) == 0
    first = ctypes.string_at(out, size.value)
    assert fn(ctypes.byref(opts), ctypes.byref(im), 6, None, ctypes.byref(out), ctypes.byref(size)) == 0
    assert ctypes.string_at(out, size.value) == first + first
    api._libc.free(out)
