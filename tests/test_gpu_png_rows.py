"""zmx_png_filter_rows_device (k_png_rows, zopfli_amd/csrc/device/zmx_png_rows.h) against the numpy reference of
tests/png_rows_cases.py — which tests/test_cpu_png_rows_cases.py holds against LodePNG — with the output at every
address mod 16 inside an allocation of guard bytes; its refusals; and zmx_png_filter_types_device against the
host-image entries and LodePNG's own search."""
import ctypes
import os
import re
import zlib

import numpy as np
import pytest
import torch

import png_rows_cases as pc
from zopfli_amd import Context

pytestmark = pytest.mark.gpu

ZMX_ERR_REFUSED = 3
IDS = [c[0] for c in pc.TABLE]


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    c = Context(0, gpu_lib)
    yield c
    c.close()


def _on_device(host, mod):
    """The bytes in device memory at `mod` bytes behind a 16-byte boundary: (the allocation, the pointer)."""
    whole = torch.zeros(mod + host.size + 16, dtype=torch.uint8, device="cuda:0")
    assert whole.data_ptr() % 16 == 0
    whole[mod:mod + host.size] = torch.from_numpy(np.ascontiguousarray(host).reshape(-1))
    return whole, whole.data_ptr() + mod


def _guarded(total, dst_mod):
    whole = torch.full((pc.GUARD + 16 + total + pc.GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    assert whole.data_ptr() % 16 == 0
    return whole, pc.GUARD + dst_mod


def _check(whole, at, want):
    got = whole.cpu().numpy()
    flat = want.reshape(-1)
    assert np.array_equal(got[at:at + flat.size], flat)
    assert np.all(got[:at] == 0xA5) and np.all(got[at + flat.size:] == 0xA5), "written outside the output"


def _rows(ctx, case, dst_mods):
    name, n, h, bw = case[:4]
    img, types = pc.make(case)
    want = pc.filter_rows(img, bw, types)
    src_mod = zlib.crc32(name.encode()) % 16
    d_img, p_img = _on_device(img, src_mod)
    d_types, p_types = _on_device(types, (src_mod * 5 + 1) % 16)
    for dst_mod in dst_mods:
        whole, at = _guarded(want.size, dst_mod)
        torch.cuda.synchronize()
        ctx.png_filter_rows_device(p_img, n, h, bw, p_types, whole.data_ptr() + at, want.size)
        _check(whole, at, want)
    assert np.array_equal(d_img.cpu().numpy()[src_mod:src_mod + img.size], img.reshape(-1)), "the image changed"
    assert np.array_equal(d_types.cpu().numpy()[(src_mod * 5 + 1) % 16:][:h], types), "the types changed"


@pytest.mark.parametrize("case", pc.TABLE, ids=IDS)
def test_rows(ctx, case):
    _rows(ctx, case, range(16))


def test_rows_stride(ctx):
    """More output than one sweep of the capped grid writes."""
    assert pc.BIG[2] * (pc.BIG[1] + 1) > pc.MAX_BLOCKS * pc.THREADS * 16
    _rows(ctx, pc.BIG, (0, 11))


def test_bad_type_names_its_row(ctx, gpu_lib):
    case = pc.TABLE[IDS.index("gradient")]
    img, types = pc.make(case)
    types = types.copy()
    types[[11, 29]] = [5, 200]
    d_img, p_img = _on_device(img, 3)
    d_types, p_types = _on_device(types, 0)
    out = torch.zeros(case[2] * (case[1] + 1), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError) as e:
        ctx.png_filter_rows_device(p_img, case[1], case[2], case[3], p_types, out)
    assert re.search(r"\brow 11\b", str(e.value)), str(e.value)
    types[[11, 29]] = [1, 2]
    d_types, p_types = _on_device(types, 0)
    ctx.png_filter_rows_device(p_img, case[1], case[2], case[3], p_types, out)   # and the next valid call is right
    assert np.array_equal(out.cpu().numpy().reshape(case[2], -1), pc.filter_rows(img, case[3], types))


def test_refusals(ctx, gpu_lib):
    """Refused before any launch (ZMX_ERR_REFUSED), the output untouched."""
    n, h, bw = 100, 20, 4
    total = h * (n + 1)
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, size=(h, n), dtype=np.uint8)
    types = (np.arange(h) % 5).astype(np.uint8)
    d_img, p_img = _on_device(img, 0)
    d_types, p_types = _on_device(types, 0)
    whole, at = _guarded(total, 0)
    out = whole.data_ptr() + at
    on_host = np.zeros(1 << 16, dtype=np.uint8)
    managed = ctypes.c_void_p()
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMallocManaged.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t, ctypes.c_uint]
    assert hip.hipMallocManaged(ctypes.byref(managed), 1 << 16, 1) == 0
    small = torch.full((4096,), 0xA5, dtype=torch.uint8, device="cuda:0")
    both = torch.zeros(h * n + total, dtype=torch.uint8, device="cuda:0")
    tall = torch.zeros(n << 16, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    refused = [
        ("null image", (0, n, h, bw, p_types, out, total)),
        ("null types", (p_img, n, h, bw, 0, out, total)),
        ("null output", (p_img, n, h, bw, p_types, 0, total)),
        ("host image", (on_host.ctypes.data, n, h, bw, p_types, out, total)),
        ("host output", (p_img, n, h, bw, p_types, on_host.ctypes.data, total)),
        ("managed image", (managed.value, n, h, bw, p_types, out, total)),
        ("managed output", (p_img, n, h, bw, p_types, managed.value, total)),
        ("image leaves its allocation", (p_img, n, 1 << 20, bw, p_types, out, (1 << 20) * (n + 1))),
        # (6.6 MB of scanlines into a tensor of 4 KiB: past the end of whatever block the allocator cut it from)
        ("output leaves its allocation", (tall.data_ptr(), n, 1 << 16, bw, tall.data_ptr(), small.data_ptr(), (n + 1) << 16)),
        ("output overlaps the image", (both.data_ptr(), n, h, bw, p_types, both.data_ptr() + h * n - 1, total)),
        ("output overlaps the types", (p_img, n, h, bw, both.data_ptr() + total - 1, both.data_ptr(), total)),
        ("capacity", (p_img, n, h, bw, p_types, out, total - 1)),
        ("linebytes 0", (p_img, 0, h, bw, p_types, out, total)),
        ("bytewidth 0", (p_img, n, h, 0, p_types, out, total)),
        ("bytewidth 9", (p_img, n, h, 9, p_types, out, total)),
        ("linebytes 2^31", (p_img, 1 << 31, 1, bw, p_types, out, (1 << 31) + 1)),
        ("height 2^31", (p_img, 1, 1 << 31, 1, p_types, out, 1 << 32)),
    ]
    if torch.cuda.device_count() >= 2:
        there = torch.zeros(h * n, dtype=torch.uint8, device="cuda:1")
        refused.append(("another device", (there.data_ptr(), n, h, bw, p_types, out, total)))
    try:
        for what, args in refused:
            with pytest.raises(RuntimeError, match="zmx_png_filter_rows_device"):
                ctx.png_filter_rows_device(*args)
                pytest.fail(what + ": not refused")
            assert gpu_lib.zmx_last_error_class() == ZMX_ERR_REFUSED, (what, gpu_lib.zmx_last_error())
        assert np.all(whole.cpu().numpy() == 0xA5) and np.all(small.cpu().numpy() == 0xA5)
        with pytest.raises(RuntimeError):       # the types' pointer is checked the same way
            ctx.png_filter_types_device(p_img, n, h, bw, "e", on_host.ctypes.data)
        assert gpu_lib.zmx_last_error_class() == ZMX_ERR_REFUSED
        with pytest.raises(RuntimeError):
            ctx.png_filter_types_device(p_img, n, h, bw, 9, p_types)
        assert gpu_lib.zmx_last_error_class() == ZMX_ERR_REFUSED
        ctx.png_filter_rows_device(p_img, n, h, bw, p_types, out, total)    # and the next valid call is right
        _check(whole, at, pc.filter_rows(img, bw, types))
    finally:
        hip.hipFree.argtypes = [ctypes.c_void_p]
        hip.hipFree(managed)


# four of tests/test_gpu_png.py's shapes: (w, h, colour type, channels, bit depth, kind)
TYPE_CASES = [(257, 33, 6, 4, 8, "gradient"), (300, 40, 2, 3, 8, "gradient"), (129, 17, 0, 1, 16, "gradient"),
              (5, 1, 2, 3, 8, "noise")]


@pytest.mark.parametrize("case", TYPE_CASES, ids=lambda c: f"{c[0]}x{c[1]}-ct{c[2]}-d{c[4]}")
def test_types_device(ctx, gpu_lib, case):
    """zmx_png_filter_types_device == zmx_png_filter_types (5, 6) and zmx_png_filter_types_brute (7, window 32768) on
    the same image from the host, == LodePNG's brute-force search at its window of 2048, and a fill for 0 .. 4."""
    from test_gpu_png import _image
    from zopfli_amd._build import PNG_FILTER_REF
    w, h, colortype, channels, depth, kind = case
    img, n = _image(np.random.default_rng(w * 131 + h), w, h, channels, depth, kind)
    bw = channels * depth // 8
    raw = img.tobytes()
    minsum, entropy, brute = (np.zeros(h, dtype=np.uint8) for _ in range(3))
    fn = gpu_lib.zmx_png_filter_types
    fn.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    assert fn(ctx.handle, raw, n, h, bw, minsum.ctypes.data, entropy.ctypes.data) == 0, ctx.error()
    fb = gpu_lib.zmx_png_filter_types_brute
    fb.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, ctypes.c_void_p]
    assert fb(ctx.handle, raw, n, h, bw, 32768, brute.ctypes.data) == 0, ctx.error()
    d_img = torch.from_numpy(img).cuda()
    d_types = torch.full((h + 32,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()

    def device_types(strategy, window=32768):
        d_types.fill_(0xA5)
        torch.cuda.synchronize()
        ctx.png_filter_types_device(d_img, n, h, bw, strategy, d_types.data_ptr() + 16, window)
        got = d_types.cpu().numpy()
        assert np.all(got[:16] == 0xA5) and np.all(got[16 + h:] == 0xA5), "written outside the types"
        return got[16:16 + h]

    for t in range(5):
        assert np.all(device_types(t) == t)
    assert np.array_equal(device_types("m"), minsum)
    assert np.array_equal(device_types("e"), entropy)
    assert np.array_equal(device_types("b"), brute)
    if os.path.exists(PNG_FILTER_REF):
        ref = ctypes.CDLL(PNG_FILTER_REF)
        ref.ref_png_filter.argtypes = [ctypes.c_char_p, ctypes.c_char_p] + [ctypes.c_uint] * 5
        ref.ref_png_filter.restype = ctypes.c_uint
        out = ctypes.create_string_buffer(h * (n + 1))
        assert ref.ref_png_filter(out, raw, w, h, colortype, depth, 7) == 0
        want = np.frombuffer(out.raw, dtype=np.uint8).reshape(h, n + 1)
        assert np.array_equal(device_types("b", 2048), want[:, 0])
        # ... and the scanlines made from them are LodePNG's
        rows = torch.zeros(h * (n + 1), dtype=torch.uint8, device="cuda:0")
        ctx.png_filter_rows_device(d_img, n, h, bw, d_types.data_ptr() + 16, rows)
        assert np.array_equal(rows.cpu().numpy().reshape(h, n + 1), want)
    assert np.array_equal(d_img.cpu().numpy(), img)
