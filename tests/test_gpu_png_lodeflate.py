"""zmx_png_deflate_sizes_device (k_png_lo_hash .. k_png_lo_parse, zopfli_amd/csrc/device/zmx_png_lodeflate.h): the
length the real LodePNG's zlib encoder gave for every buffer of tests/png_trial_cases.py (tests/golden/png_trials.json,
window 8192) — one, two, three bytes; the window's edge with copies at 8191, 8192 and 8193; one deflate block against
two; a copy and a zero run over block ends; eight blocks; the block size's cap; lazy matches taken, beaten and rolled back
at a block's end; a match of 3 at 4096 and 4097; a match of 258 — eight of them in one call as in eight, other windows
against the CPU run of the kernels' rules, and the refusals, which leave the output as it was.  Only the size is compared
here; the per-position arrays and every block's symbol counts at short tile lengths, and windows other than 8192 against
LodePNG itself, are tests/test_gpu_png_lodeflate_seams.py's."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import png_trial_cases as tc
from zopfli_amd import Context
from zopfli_amd._build import ROOT

pytestmark = pytest.mark.gpu

ZMX_ERR_REFUSED = 3


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    c = Context(0, gpu_lib)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gold():
    return tc.golden()


def _on_device(a):
    d = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return d


@pytest.mark.parametrize("name", tc.BUFFER_IDS)
def test_size_is_lodepngs(ctx, gpu_lib, gold, name):
    d = _on_device(tc.buffer(name))
    assert ctx.png_deflate_sizes_device([d], tc.WINDOW) == [gold["buffers"][name]], name
    assert np.array_equal(d.cpu().numpy(), tc.buffer(name)), "the buffer changed"


def test_eight_buffers_in_one_call(ctx, gold):
    bufs = [_on_device(tc.buffer(name)) for name in tc.MIXED_CALL]
    want = [gold["buffers"][name] for name in tc.MIXED_CALL]
    singles = [ctx.png_deflate_sizes_device([d], tc.WINDOW)[0] for d in bufs]
    assert singles == want
    assert ctx.png_deflate_sizes_device(bufs, tc.WINDOW) == singles
    order = [5, 2, 7, 0, 3, 6, 1, 4]
    assert ctx.png_deflate_sizes_device([bufs[i] for i in order], tc.WINDOW) == [singles[i] for i in order]
    # slices of one allocation, at odd addresses
    whole = torch.zeros(sum(len(b) for b in bufs) + 3 * len(bufs), dtype=torch.uint8, device="cuda:0")
    at, ranges = 1, []
    for b in bufs:
        whole[at:at + len(b)] = b
        ranges.append((whole.data_ptr() + at, len(b)))
        at += len(b) + 3
    torch.cuda.synchronize()
    assert ctx.png_deflate_sizes_device(ranges, tc.WINDOW) == singles


def test_other_windows_against_the_cpu_run(ctx, tmp_path):
    """Windows 256 .. 32768 (maxchainlength and maxlazymatch change at 8192): the device against the same rules run on the
    CPU by tests/hostlib/png_lodeflate_print.cc, which tests/test_cpu_png_trial_cases.py holds to LodePNG at 8192."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "hostlib"), "-f", "png_lodeflate.mk"])
    exe = os.path.join(ROOT, "tests", "_build", "png_lodeflate_print")
    names = ["period-8193-x4", "block-65537", "hash0-nonzero", "lazy-beaten"]
    paths = []
    for i, name in enumerate(names):
        paths.append(str(tmp_path / f"b{i}.bin"))
        tc.buffer(name).tofile(paths[-1])
    bufs = [_on_device(tc.buffer(name)) for name in names]
    for window in (256, 2048, 32768):
        want = [int(v) for v in subprocess.check_output([exe, "size", str(window), "262144"] + paths, text=True).split()]
        assert ctx.png_deflate_sizes_device(bufs, window) == want, window


def test_refusals_leave_the_sizes_untouched(ctx, gpu_lib):
    lib = gpu_lib
    fn = lib.zmx_png_deflate_sizes_device
    fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.c_uint,
                   ctypes.POINTER(ctypes.c_uint64)]
    fn.restype = ctypes.c_int
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    on_host = np.zeros(4096, dtype=np.uint8)
    torch.cuda.synchronize()
    p = d.data_ptr()

    def call(handle, n, ptrs, sizes, window, out=True):
        res = (ctypes.c_uint64 * 2)(111, 222)
        rc = fn(handle, n, (ctypes.c_void_p * 2)(*ptrs) if ptrs is not None else None,
                (ctypes.c_size_t * 2)(*sizes) if sizes is not None else None, window, res if out else None)
        return rc, list(res)

    refused = [
        ("no context", (None, 2, (p, p), (10, 10), 8192)),
        ("no buffers", (ctx.handle, 0, (p, p), (10, 10), 8192)),
        ("null pointers", (ctx.handle, 2, None, (10, 10), 8192)),
        ("null sizes", (ctx.handle, 2, (p, p), None, 8192)),
        ("a null buffer", (ctx.handle, 2, (p, None), (10, 10), 8192)),
        ("a size of 0", (ctx.handle, 2, (p, p), (10, 0), 8192)),
        ("window 0", (ctx.handle, 2, (p, p), (10, 10), 0)),
        ("window 3000", (ctx.handle, 2, (p, p), (10, 10), 3000)),
        ("window 65536", (ctx.handle, 2, (p, p), (10, 10), 65536)),
        ("host memory", (ctx.handle, 2, (p, on_host.ctypes.data), (10, 10), 8192)),
        ("a range that leaves its allocation", (ctx.handle, 2, (p, p + 4000), (10, 1 << 30), 8192)),
    ]
    for what, args in refused:
        rc, res = call(*args)
        assert rc != 0 and lib.zmx_last_error_class() == ZMX_ERR_REFUSED, (what, lib.zmx_last_error())
        assert res == [111, 222], what
    rc, _ = call(ctx.handle, 2, (p, p), (10, 10), 8192, out=False)
    assert rc != 0 and lib.zmx_last_error_class() == ZMX_ERR_REFUSED
    # and the next valid call is right: 4096 zeros twice
    rc, res = call(ctx.handle, 2, (p, p), (4096, 4096), 8192)
    assert rc == 0 and res[0] == res[1] == ctx.png_deflate_sizes_device([d], 8192)[0]
