"""zopflipng's --lossy_transparent and --lossy_8bit on images in device memory.  zmx_png_lossy_transparent_device is held
against the numpy model of tests/png_lossy_cases.py on every case — the image and the info, out of place at every
alignment of the output between guard bytes, the image moving the other way, and in place.  The four _lossy entries are
held, for the entries' cases and the strategies 0 4 m e b, against the file put together in Python from the model (the
rewritten pixels, png_color_cases' mode and conversion, the numpy-filtered scanlines with the types of the host-image
row searches, the library's host ZopfliCompress(ZLIB)) and against the all-reference zopflipng with the same flags
(oracle/_ref/zopflipng_ref, where it was built).  numiterations 2 throughout."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import png_color_cases as cc
import png_encode_cases as ec
import png_lossy_cases as lc
from png_rows_cases import filter_rows
from test_gpu_png_optimize import _types
from zopfli_amd import Context, ZopfliOptions, api
from zopfli_amd._build import PNG_REF

pytestmark = pytest.mark.gpu

ZMX_ERR_REFUSED = 3
ITERATIONS = 2
STRATEGIES = [0, 4, 5, 6, 7]
GUARD = 256
NO_INDEX = (1 << 64) - 1


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    c = Context(0, gpu_lib)
    yield c
    c.close()


def _info(i):
    return {"mode": i.mode, "partial_alpha": i.partial_alpha, "numcolors": i.numcolors, "fill": (i.fill_r, i.fill_g, i.fill_b),
            "first_transparent": None if i.first_transparent == NO_INDEX else i.first_transparent}


def _placed(flat, mod):
    """The bytes `mod` bytes behind a 256-byte boundary of a device buffer of their own: (buffer, offset)."""
    buf = torch.empty(16 + flat.size, dtype=torch.uint8, device="cuda:0")
    buf[mod:mod + flat.size] = torch.from_numpy(np.array(flat))
    return buf, mod


def _step(ctx, case, src_mod, dst_mod, inplace=False):
    """(info, rewritten image, guards held, source untouched) of one call."""
    name, w, h, ct, depth = case
    flat = lc.pixels(case).reshape(-1)
    n = flat.size
    src, at = _placed(flat, src_mod)
    image = (src.data_ptr() + at, w, h, ct, depth)
    if inplace:
        whole = torch.full((GUARD + 16 + n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
        to = GUARD + dst_mod
        whole[to:to + n] = torch.from_numpy(np.array(flat))
        torch.cuda.synchronize()
        info = ctx.png_lossy_transparent_device((whole.data_ptr() + to, w, h, ct, depth), whole.data_ptr() + to, n)
    else:
        whole = torch.full((GUARD + 16 + n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
        to = GUARD + dst_mod
        torch.cuda.synchronize()
        info = ctx.png_lossy_transparent_device(image, whole.data_ptr() + to, n)
    torch.cuda.synchronize()
    host = whole.cpu().numpy()
    guards = bool(np.all(host[:to] == 0xA5) and np.all(host[to + n:] == 0xA5))
    untouched = bool(np.array_equal(src.cpu().numpy()[at:at + n], flat))
    return _info(info), host[to:to + n].reshape(h, -1), guards, untouched


def _check(got, case, what):
    info, img, guards, untouched = got
    want_info, want = lc.model(case)
    assert info == want_info, (case[0], what, info, want_info)
    assert np.array_equal(img, want), (case[0], what)
    assert guards, (case[0], what, "written outside the output")
    assert untouched, (case[0], what, "the source changed")


@pytest.mark.parametrize("case", [c for c in lc.CASES if c[0] not in lc.SWEEP_CASES], ids=[n for n in lc.IDS if n not in lc.SWEEP_CASES])
def test_step(ctx, case):
    """Every alignment of the output, the image moving the other way, and in place (the large case: three of each)."""
    for k in (range(16) if case[0] not in lc.LARGE else (0, 5, 10)):
        _check(_step(ctx, case, (7 * k + 3) % 16, k), case, ("out of place", k))
        _check(_step(ctx, case, 0, k, inplace=True), case, ("in place", k))


def test_step_beyond_a_sweep(ctx):
    """A few million pixels, just beyond one sweep of a full launch: the transparent runs cross the sweep's edge."""
    case = lc.case("run-sweep")
    _check(_step(ctx, case, 0, 4), case, "out of place")
    _check(_step(ctx, case, 0, 0, inplace=True), case, "in place")


def test_colour_types_without_alpha(ctx):
    """Grey and RGB have nothing transparent: mode 0 and a copy."""
    for ct, depth in ((0, 8), (2, 8), (2, 16)):
        w, h = 37, 11
        flat = np.random.default_rng(ct + depth).integers(0, 256, size=w * h * ec.CHANNELS[ct] * depth // 8, dtype=np.uint8)
        d_img = torch.from_numpy(flat).cuda()
        d_out = torch.full((flat.size + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        info = _info(ctx.png_lossy_transparent_device((d_img.data_ptr(), w, h, ct, depth), d_out.data_ptr() + 3, flat.size))
        assert info == {"mode": 0, "partial_alpha": 0, "numcolors": 0, "fill": (0, 0, 0), "first_transparent": None}
        host = d_out.cpu().numpy()
        assert np.array_equal(host[3:3 + flat.size], flat) and np.all(host[:3] == 0xA5) and np.all(host[3 + flat.size:] == 0xA5)


# ---- the entries
def _file(ctx, lib, img, w, h, ct, depth, mode, strategy):
    """The file of the (h, linebytes) image in `mode` (None: as it is), put together in Python."""
    if mode is None:
        bw = ec.CHANNELS[ct] * depth // 8
        scan = filter_rows(img, bw, _types(ctx, lib, img, bw, strategy))
        return ec.assemble((w, h, ct, depth), api.compress(scan.tobytes(), api.FORMAT_ZLIB, ZopfliOptions(ITERATIONS), lib=lib))
    conv = np.ascontiguousarray(cc.convert(cc.expand(img, w, h, ct, depth), depth, w, h, mode))
    scan = filter_rows(conv, cc.bytewidth(mode), _types(ctx, lib, conv, cc.bytewidth(mode), strategy))
    return cc.assemble(w, h, mode, api.compress(scan.tobytes(), api.FORMAT_ZLIB, ZopfliOptions(ITERATIONS), lib=lib))


def _expected(ctx, lib, case, flags, optimize, strategy):
    """(file, its mode: None for the encode entry, whether the second try replaced the first: None where none is made)."""
    name, w, h, ct, depth = case
    img, d = lc.prepared(case, flags, optimize)
    if not optimize:
        return _file(ctx, lib, img, w, h, ct, d, None, strategy), None, None
    rgba, st, mode = lc.reduced(img, w, h, ct, d)
    first = _file(ctx, lib, img, w, h, ct, d, mode, strategy)
    if mode["colortype"] != 3 or len(first) >= cc.RETRY_BELOW:
        return first, mode, None
    again = cc.retry_mode(st, w * h)
    second = _file(ctx, lib, img, w, h, ct, d, again, strategy)
    return (second, again, True) if len(second) < len(first) else (first, mode, False)


REF_FLAGS = {0: [], 1: ["--lossy_transparent"], 2: ["--lossy_8bit"], 3: ["--lossy_transparent", "--lossy_8bit"]}


def _reference(tmp_path, case, flags, optimize, strategy):
    """The all-reference zopflipng's file, or None where it was not built."""
    if not os.path.exists(PNG_REF):
        return None
    name, w, h, ct, depth = case
    src, dst = str(tmp_path / "in.png"), str(tmp_path / "ref.png")
    with open(src, "wb") as f:
        f.write(ec.plain_png((w, h, ct, depth), filter_rows(lc.pixels(case), ec.CHANNELS[ct] * depth // 8, np.zeros(h, dtype=np.uint8))))
    r = subprocess.run([PNG_REF, "-y", "--always_zopflify", f"--iterations={ITERATIONS}", f"--filters={ec.STRATEGY_LETTERS[strategy]}",
                        *([] if optimize else ["--keepcolortype"]), *REF_FLAGS[flags], src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-1000:])
    with open(dst, "rb") as f:
        return f.read()


def _call(lib, case, d_img, strategy, flags, optimize):
    name, w, h, ct, depth = case
    fn = api.png_optimize_device if optimize else api.png_encode_device
    return fn((d_img.data_ptr(), w, h, ct, depth), strategy, ZopfliOptions(ITERATIONS), lib=lib, lossy_transparent=bool(flags & 1),
              lossy_8bit=bool(flags & 2))


def _call_lossy(lib, case, d_img, strategy, flags, optimize):
    """The _lossy symbol itself, lossy = 0 included."""
    name, w, h, ct, depth = case
    fn = lib.zmx_png_optimize_device_lossy if optimize else lib.zmx_png_encode_device_lossy
    fn.argtypes = [ctypes.POINTER(ZopfliOptions), ctypes.POINTER(api.PngImage), ctypes.c_int, ctypes.c_char_p, ctypes.c_uint,
                   ctypes.POINTER(api._u8p), ctypes.POINTER(ctypes.c_size_t)]
    fn.restype = ctypes.c_int
    out, size = api._u8p(), ctypes.c_size_t(0)
    im = api.PngImage(d_img.data_ptr(), w, h, ct, depth)
    assert fn(ctypes.byref(ZopfliOptions(ITERATIONS)), ctypes.byref(im), strategy, None, flags, ctypes.byref(out), ctypes.byref(size)) == 0, \
        lib.zmx_last_error()
    return api._take(out, size)


def _on_device(case):
    d_img = torch.from_numpy(lc.pixels(case).copy()).cuda()
    torch.cuda.synchronize()
    return d_img


@pytest.mark.parametrize("name", lc.ENTRY_CASES)
def test_entries(ctx, gpu_lib, tmp_path, name):
    case = lc.case(name)
    _, w, h, ct, depth = case
    d_img = _on_device(case)
    for optimize in (False, True):
        for flags in (1, 2, 3):
            for strategy in STRATEGIES:
                png = _call(gpu_lib, case, d_img, strategy, flags, optimize)
                assert api.last_input_traffic(gpu_lib)[0] == 0, "pixels went host to device"
                want, mode, retried = _expected(ctx, gpu_lib, case, flags, optimize, strategy)
                tags = [t for t, _ in ec.chunks(png)]
                assert tags == ([b"IHDR", b"IDAT", b"IEND"] if mode is None else cc.expected_chunks(mode)), (name, flags, strategy)
                assert png == want, (name, optimize, flags, strategy)
                ref = _reference(tmp_path, case, flags, optimize, strategy)
                assert ref is None or png == ref, (name, optimize, flags, strategy, "zopflipng_ref")
                if optimize and strategy == 0:
                    first_mode = lc.reduced(lc.prepared(case, flags, True)[0], w, h, ct, lc.prepared(case, flags, True)[1])[2]
                    assert lc.mode_tuple(first_mode) == lc.OPTIMIZE_EXPECT[name][flags], (name, flags)
                    if flags == 1 and name in lc.RETRY_EXPECT:
                        assert retried == lc.RETRY_EXPECT[name], (name, "the second try")
    # tRNS and PLTE appear only with the flag, where the table says so
    for flags in (0, 1):
        tags = [t for t, _ in ec.chunks(_call_lossy(gpu_lib, case, d_img, 0, flags, True))]
        expect = lc.OPTIMIZE_EXPECT[name][flags]
        if expect[0] != 3:
            assert (b"tRNS" in tags) == (expect[3] is not None) and b"PLTE" not in tags, (name, flags)
    assert np.array_equal(d_img.cpu().numpy(), lc.pixels(case)), "the caller's image changed"


@pytest.mark.parametrize("name", lc.ENTRY_CASES)
def test_flags_that_do_nothing(gpu_lib, name):
    """lossy = 0 is the plain entry's file; _8BIT does nothing to the encode entry, _TRANSPARENT alone nothing to a 16-bit
    image, either nothing to an image without a transparent pixel."""
    case = lc.case(name)
    _, w, h, ct, depth = case
    d_img = _on_device(case)
    for strategy in (0, 6):
        for optimize in (False, True):
            plain = _call(gpu_lib, case, d_img, strategy, 0, optimize)
            assert _call_lossy(gpu_lib, case, d_img, strategy, 0, optimize) == plain, (name, optimize, "lossy = 0")
            same = []
            if not optimize:
                same.append(2)
            if depth == 16:
                same.append(1)
            if depth == 8 and optimize:
                same.append(2)
            if name == "no-transparent":
                same += [1, 2, 3]
            if name == "idempotent":
                same.append(1)
            for flags in same:
                assert _call_lossy(gpu_lib, case, d_img, strategy, flags, optimize) == plain, (name, optimize, flags)
            if not optimize and depth == 8:
                assert _call_lossy(gpu_lib, case, d_img, strategy, 3, optimize) == _call_lossy(gpu_lib, case, d_img, strategy, 1, optimize)


def test_batches_equal_singles(gpu_lib):
    cases = [lc.case(n) for n in lc.ENTRY_CASES]
    imgs = [_on_device(c) for c in cases]
    images = [(d.data_ptr(),) + tuple(c[1:]) for c, d in zip(cases, imgs)]
    order = [(7 * i + 3) % len(cases) for i in range(len(cases))]
    assert sorted(order) == list(range(len(cases)))
    for optimize, batch in ((False, api.png_encode_device_batch), (True, api.png_optimize_device_batch)):
        for strategy, flags in ((0, 1), (6, 3)):
            kw = {"lossy_transparent": bool(flags & 1), "lossy_8bit": bool(flags & 2)}
            singles = [_call(gpu_lib, c, d, strategy, flags, optimize) for c, d in zip(cases, imgs)]
            if optimize:
                # (both kinds of second try are in: one that wins and one that loses)
                kinds = [ec.chunks(s)[0][1][9] for s in singles]
                assert kinds[lc.ENTRY_CASES.index("retry-wins")] in (2, 6) and kinds[lc.ENTRY_CASES.index("retry-loses")] == 3
            assert batch(images, strategy, ZopfliOptions(ITERATIONS), lib=gpu_lib, **kw) == singles
            assert api.last_input_traffic(gpu_lib)[0] == 0
            assert batch([images[i] for i in order], strategy, ZopfliOptions(ITERATIONS), lib=gpu_lib, **kw) == [singles[i] for i in order]
        assert batch([], "e", lib=gpu_lib, lossy_transparent=True) == []
    for c, d in zip(cases, imgs):
        assert np.array_equal(d.cpu().numpy(), lc.pixels(c)), "a caller's image changed"


def _managed(nbytes):
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMallocManaged.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t, ctypes.c_uint]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    p = ctypes.c_void_p()
    assert hip.hipMallocManaged(ctypes.byref(p), nbytes, 1) == 0
    return p.value, lambda: hip.hipFree(p)


def test_step_refusals_write_nothing(ctx, gpu_lib):
    """Refused before any launch.  Memory of another device is tried only where a second device is visible: on a machine
    with one GPU that refusal is not exercised here (the check is CheckDevicePointer's, shared with the other device
    entries)."""
    lib = gpu_lib
    d_img = torch.zeros(64 * 64 * 8, dtype=torch.uint8, device="cuda:0")
    d_out = torch.full((64 * 64 * 8,), 0xA5, dtype=torch.uint8, device="cuda:0")
    on_host = np.zeros(4096, dtype=np.uint8)
    managed, free_managed = _managed(4096)
    torch.cuda.synchronize()
    p, q = d_img.data_ptr(), d_out.data_ptr()
    fn = lib.zmx_png_lossy_transparent_device
    fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(api.PngImage), ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(api.PngLossyInfo)]
    fn.restype = ctypes.c_int
    good = (p, 16, 16, 6, 8)
    refused = [
        ("width 0", (p, 0, 16, 6, 8), q, 4096), ("height 0", (p, 16, 0, 6, 8), q, 4096), ("palette input", (p, 16, 16, 3, 8), q, 4096),
        ("colour type 1", (p, 16, 16, 1, 8), q, 4096), ("depth 4", (p, 16, 16, 4, 4), q, 4096), ("null pixels", (None, 16, 16, 6, 8), q, 4096),
        ("host pixels", (on_host.ctypes.data, 16, 16, 6, 8), q, 4096), ("pixels leave their allocation", (p, 16384, 16384, 6, 16), q, 1 << 40),
        ("2^32 pixels", (p, 65536, 65536, 4, 8), q, 1 << 40),
        ("a capacity one byte short", good, q, 16 * 16 * 4 - 1), ("null output", good, None, 4096), ("host output", good, on_host.ctypes.data, 4096),
        ("managed output", good, managed, 4096), ("output overlaps the image's end", good, p + 16 * 16 * 4 - 1, 4096),
        ("output overlaps the image's start", (p + 512, 16, 16, 6, 8), p, 4096), ("output one byte into the image", good, p + 1, 4096),
    ]
    if torch.cuda.device_count() > 1:
        other = torch.zeros(4096, dtype=torch.uint8, device="cuda:1")
        refused.append(("another device's memory", good, other.data_ptr(), 4096))
    try:
        for what, image, out, capacity in refused:
            im = api.PngImage(*image)
            info = api.PngLossyInfo()
            ctypes.memset(ctypes.byref(info), 0x5A, ctypes.sizeof(info))
            assert fn(ctx.handle, ctypes.byref(im), out, capacity, ctypes.byref(info)) != 0, what
            assert lib.zmx_last_error_class() == ZMX_ERR_REFUSED, (what, lib.zmx_last_error())
            assert bytes(info) == b"\x5a" * ctypes.sizeof(info), what
        assert fn(None, ctypes.byref(api.PngImage(*good)), q, 4096, None) != 0
        torch.cuda.synchronize()
        assert bool(torch.all(d_out == 0xA5)) and bool(torch.all(d_img == 0)) and not on_host.any(), "a refused call wrote"
    finally:
        free_managed()
    # and the valid call next to them works, without an info too: 256 transparent black pixels stay what they are
    assert fn(ctx.handle, ctypes.byref(api.PngImage(*good)), q, 16 * 16 * 4, None) == 0, lib.zmx_last_error()
    torch.cuda.synchronize()
    assert bool(torch.all(d_out[:16 * 16 * 4] == 0)) and bool(torch.all(d_out[16 * 16 * 4:] == 0xA5))


def test_entry_refusals_leave_out_untouched(gpu_lib):
    """ZMX_ERR_REFUSED before anything runs; (*out, *outsize) as they were, in the batches every one of them."""
    lib = gpu_lib
    d_img = torch.zeros(64 * 64 * 8, dtype=torch.uint8, device="cuda:0")
    on_host = np.zeros(4096, dtype=np.uint8)
    torch.cuda.synchronize()
    p = d_img.data_ptr()
    single = [ctypes.POINTER(ZopfliOptions), ctypes.POINTER(api.PngImage), ctypes.c_int, ctypes.c_char_p, ctypes.c_uint,
              ctypes.POINTER(api._u8p), ctypes.POINTER(ctypes.c_size_t)]
    many = [ctypes.POINTER(ZopfliOptions), ctypes.c_size_t, ctypes.POINTER(api.PngImage), ctypes.c_int, ctypes.c_uint,
            ctypes.POINTER(api._u8p), ctypes.POINTER(ctypes.c_size_t)]
    opts = ZopfliOptions(ITERATIONS)
    good_image = (p, 16, 16, 6, 8)
    refused = [
        ("lossy 4", good_image, 6, None, 4), ("lossy 7", good_image, 6, None, 7), ("lossy 2^31", good_image, 6, None, 1 << 31),
        ("width 0", (p, 0, 16, 6, 8), 6, None, 1), ("height 0", (p, 16, 0, 6, 8), 6, None, 1), ("palette input", (p, 16, 16, 3, 8), 6, None, 1),
        ("colour type 1", (p, 16, 16, 1, 8), 6, None, 3), ("depth 4", (p, 16, 16, 0, 4), 6, None, 3), ("depth 32", (p, 16, 16, 0, 32), 6, None, 3),
        ("strategy 9", good_image, 9, None, 1), ("strategy -1", good_image, -1, None, 1), ("predefined without types", good_image, 8, None, 1),
        ("predefined type 5", good_image, 8, bytes([0] * 15 + [5]), 1), ("null pixels", (None, 16, 16, 6, 8), 6, None, 1),
        ("host pixels", (on_host.ctypes.data, 16, 16, 6, 8), 6, None, 1), ("pixels leave their allocation", (p, 16384, 16384, 6, 16), 6, None, 3),
    ]
    sentinel = api._libc.malloc(8)
    ctypes.memmove(sentinel, b"abc", 3)
    try:
        for stem in ("zmx_png_encode_device", "zmx_png_optimize_device"):
            fn, fb = getattr(lib, stem + "_lossy"), getattr(lib, stem + "_batch_lossy")
            fn.argtypes, fn.restype, fb.argtypes, fb.restype = single, ctypes.c_int, many, ctypes.c_int
            # (2^32 pixels: the optimize entries refuse any such image, the encode entries one _TRANSPARENT would rewrite)
            cases = refused + [("2^32 pixels", (p, 65536, 65536, 4, 8), 6, None, 1)]
            cases += [("2^32 grey pixels", (p, 65536, 65536, 0, 8), 6, None, 1)] if "optimize" in stem else []
            for what, image, strategy, types, lossy in cases:
                out, size = ctypes.cast(sentinel, api._u8p), ctypes.c_size_t(3)
                im = api.PngImage(*image)
                assert fn(ctypes.byref(opts), ctypes.byref(im), strategy, types, lossy, ctypes.byref(out), ctypes.byref(size)) != 0, (stem, what)
                assert lib.zmx_last_error_class() == ZMX_ERR_REFUSED, (stem, what, lib.zmx_last_error())
                assert not what.startswith("2^32") or (b"2^32" in lib.zmx_last_error() and stem.encode() in lib.zmx_last_error()), what
                assert ctypes.cast(out, ctypes.c_void_p).value == sentinel and size.value == 3, (stem, what)
                # the same image in the middle of a batch: no out[i] changes
                good = api.PngImage(*good_image)
                arr = (api.PngImage * 3)(good, im, good)
                outs = (api._u8p * 3)(*[ctypes.cast(sentinel, api._u8p)] * 3)
                sizes = (ctypes.c_size_t * 3)(3, 3, 3)
                assert fb(ctypes.byref(opts), 3, arr, strategy, lossy, outs, sizes) != 0, (stem, what)
                assert lib.zmx_last_error_class() == ZMX_ERR_REFUSED, (stem, what, lib.zmx_last_error())
                assert not what.startswith("2^32") or b"2^32" in lib.zmx_last_error(), what
                assert all(ctypes.cast(outs[i], ctypes.c_void_p).value == sentinel and sizes[i] == 3 for i in range(3)), (stem, what)
            assert ctypes.string_at(sentinel, 3) == b"abc"
            # and the next valid call appends to what it is given
            out, size = api._u8p(), ctypes.c_size_t(0)
            im = api.PngImage(*good_image)
            assert fn(ctypes.byref(opts), ctypes.byref(im), 6, None, 3, ctypes.byref(out), ctypes.byref(size)) == 0, lib.zmx_last_error()
            first = ctypes.string_at(out, size.value)
            assert fn(ctypes.byref(opts), ctypes.byref(im), 6, None, 3, ctypes.byref(out), ctypes.byref(size)) == 0
            assert ctypes.string_at(out, size.value) == first + first
            api._libc.free(out)
    finally:
        api._libc.free(sentinel)
    assert bool(torch.all(d_img == 0)), "the caller's image changed"
