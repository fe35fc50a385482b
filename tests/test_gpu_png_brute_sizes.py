"""k_png_brute (zopfli_amd/csrc/device/zmx_png_brute.h) size by size: zmx_internal_png_brute_sizes hands out the five zlib
sizes the kernel wrote for every row, its bit counts before rounding and k_png_brute_pick's types.  On the cases of
tests/png_brute_size_cases.py — rows on either side of the LDS / scratch boundary (16839 bytes) and of the raised LDS limit
(7281), rows around and beyond every window from 256 to 32768, windows from 1 to 32768, chunks of 1024 positions that end
at, before and behind the row's end, rows of one to three bytes, pixels of 1 to 8 bytes — every job's bits and bytes must be
the real LodePNG's (oracle/_ref/libpng_brute_ref.so: filterScanline, encodeLZ77, lodepng_zlib_compress), and the model's
(tools/models/png_brute_model.h) wherever tests/test_cpu_png_brute_sizes.py runs it.  Rows of up to 5000 bytes run once
more with the per-position arrays forced into the global scratch, and one image runs on grids of 1, 2 and 3 workgroups,
so that a workgroup's next job meets what the last one left in `head`, `s_headz` and the arrays.  No tolerance anywhere."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import png_brute_size_cases as bc
from zopfli_amd import Context
from zopfli_amd._build import PNG_BRUTE_REF, ROOT

pytestmark = pytest.mark.gpu

ZMX_ERR_REFUSED = 3


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    c = Context(0, gpu_lib)
    yield c
    c.close()


@pytest.fixture(scope="module")
def exe():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "hostlib"), "-f", "png_brute.mk"])
    return os.path.join(ROOT, "tests", "_build", "png_brute_print")


@pytest.fixture(scope="module")
def ref():
    assert os.path.exists(PNG_BRUTE_REF), "oracle/_ref/libpng_brute_ref.so not built"
    return bc.ref_library(PNG_BRUTE_REF)


def _probe(ctx, case, force_scratch=0, max_workgroups=0):
    return ctx.png_brute_sizes(case.image(), case.linebytes, case.height, case.bytewidth, case.window, force_scratch, max_workgroups)


@pytest.mark.parametrize("name", bc.CASE_IDS)
def test_device_sizes_and_bits_are_lodepngs(ctx, ref, exe, tmp_path, name):
    case = bc.CASES[name]
    want_size, want_bits, reach, want_types = bc.ref_run(ref, case)
    case.check(reach)
    model = bc.model_run(exe, tmp_path, case) if case.model else None
    runs = []
    for force_scratch, max_workgroups in case.knobs:
        where = (name, "force_scratch", force_scratch, "max_workgroups", max_workgroups)
        sizes, bits, types = _probe(ctx, case, force_scratch, max_workgroups)
        assert sizes.shape == bits.shape == (case.height, 5) and types.shape == (case.height,)
        for what, got, want in (("bits", bits, want_bits), ("bytes", sizes, want_size)):
            bad = bc.mismatches(got, want)
            print(where, what, "differ in", int((got != want).sum()), "of", got.size, "jobs")
            assert not bad, (where, what, "(row, type, device, LodePNG)", bad)
        assert np.array_equal(sizes, 6 + (bits + 7) // 8), (where, bc.mismatches(sizes, 6 + (bits + 7) // 8))
        assert np.array_equal(types, bc.first_smallest(sizes)), (where, types.tolist())
        assert np.array_equal(types, want_types), (where, "device", types.tolist(), "LodePNG's filter()", want_types.tolist())
        if model is not None:
            assert np.array_equal(sizes, model[0]) and np.array_equal(bits, model[1]), (where, "(row, type, device, model)", bc.mismatches(bits, model[1]))
        runs.append((sizes, bits, types))
    for other in runs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(runs[0], other)), (name, "the runs differ among themselves")


def test_public_entries_run_the_scratch_path(ctx, gpu_lib, ref):
    """zmx_png_filter_types_brute and zmx_png_filter_types_device with ZMX_PNG_FILTER_BRUTE on rows of 16840 bytes, the first
    length whose per-position arrays live in the global scratch: the probe's types, which are LodePNG's."""
    case = bc.CASES[f"lds-edge-{bc.LDS_LAST + 1}-w32768"]
    assert bc.row_bytes(case.linebytes) > 148 * 1024 >= bc.row_bytes(case.linebytes - 1)
    _, _, _, want = bc.ref_run(ref, case)
    _, _, types = _probe(ctx, case)
    assert np.array_equal(types, want)
    img = case.image()
    fn = gpu_lib.zmx_png_filter_types_brute
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, ctypes.c_void_p]
    fn.restype = ctypes.c_int
    out = np.full(case.height, 255, dtype=np.uint8)
    assert fn(ctx.handle, img.ctypes.data, case.linebytes, case.height, case.bytewidth, case.window, out.ctypes.data) == 0, ctx.error()
    assert np.array_equal(out, types)
    d_img = torch.from_numpy(np.array(img)).cuda()
    d_types = torch.full((case.height,), 255, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.png_filter_types_device(d_img, case.linebytes, case.height, case.bytewidth, "b", d_types, case.window)
    assert np.array_equal(d_types.cpu().numpy(), types)
    assert np.array_equal(d_img.cpu().numpy(), img), "the image changed"


def test_refusals_of_the_probe(ctx, gpu_lib):
    """What zmx_png_filter_types_brute refuses, a knob that is neither 0 nor 1 and a missing output: ZMX_ERR_REFUSED, the
    outputs untouched; then a call that is taken."""
    case = bc.CASES["tiny-5"]
    img = case.image()
    fn = gpu_lib.zmx_internal_png_brute_sizes
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, ctypes.c_int,
                   ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    fn.restype = ctypes.c_int
    jobs = 5 * case.height
    sizes, bits = np.full(jobs, 111, dtype=np.uint64), np.full(jobs, 222, dtype=np.uint64)
    types = np.full(case.height, 99, dtype=np.uint8)

    def call(handle=ctx.handle, linebytes=case.linebytes, bytewidth=case.bytewidth, window=case.window, force=0, s=sizes, b=bits, t=types):
        return fn(handle, img.ctypes.data, linebytes, case.height, bytewidth, window, force, 0,
                  None if s is None else s.ctypes.data, None if b is None else b.ctypes.data, None if t is None else t.ctypes.data)

    refused = [("no context", dict(handle=None)), ("window 3", dict(window=3)), ("window 65536", dict(window=65536)), ("window 0", dict(window=0)),
               ("force_scratch 2", dict(force=2)), ("force_scratch -1", dict(force=-1)), ("no sizes", dict(s=None)), ("no bits", dict(b=None)),
               ("no types", dict(t=None)), ("rows of 0 bytes", dict(linebytes=0)), ("pixels of 9 bytes", dict(bytewidth=9))]
    for what, args in refused:
        assert call(**args) != 0, what
        assert gpu_lib.zmx_last_error_class() == ZMX_ERR_REFUSED, (what, gpu_lib.zmx_last_error())
        assert (sizes == 111).all() and (bits == 222).all() and (types == 99).all(), what
    assert call() == 0, ctx.error()
    want = _probe(ctx, case)
    assert np.array_equal(sizes.reshape(-1, 5), want[0]) and np.array_equal(bits.reshape(-1, 5), want[1]) and np.array_equal(types, want[2])
