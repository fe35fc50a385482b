"""k_png_lo_hash .. k_png_lo_parse (zopfli_amd/csrc/device/zmx_png_lodeflate.h) word by word at tile seams:
zmx_internal_png_lodeflate_arrays runs zmx_png_deflate_sizes_device's kernels at a caller's tile length and hands out what
they left in device memory — HC, ZC and LD of every position, the 316 symbol counts and the extra bits of every deflate
block.  On the cases of tests/png_lodeflate_seam_cases.py (links that ask several tables back, KEEP walks through words
other lanes are resolving, zero-run keys over seams, tiles and chunks of one position, a buffer behind another, a lazy
match over the parse's LDS refill) they must equal the CPU run of the same rules (tests/hostlib/png_lodeflate_print.cc)
at the same tile length, and the counts must be the real LodePNG's (oracle/_ref/libpng_lodeflate_ref.so), which
tests/test_cpu_png_lodeflate_seams.py also holds the CPU run to, at windows from 256 to 32768."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import png_lodeflate_seam_cases as sc
from zopfli_amd import Context
from zopfli_amd._build import PNG_LODEFLATE_REF, ROOT

pytestmark = pytest.mark.gpu

ZMX_ERR_REFUSED = 3
ARRAYS = ("HC", "ZC", "LD")
GUARDED = [n for n in sc.CASE_IDS if n.startswith("never-seen-")] + ["zero-runs-over-seams"]


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    c = Context(0, gpu_lib)
    yield c
    c.close()


@pytest.fixture(scope="module")
def exe():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "hostlib"), "-f", "png_lodeflate.mk"])
    return os.path.join(ROOT, "tests", "_build", "png_lodeflate_print")


@pytest.fixture(scope="module")
def ref():
    assert os.path.exists(PNG_LODEFLATE_REF), "oracle/_ref/libpng_lodeflate_ref.so not built"
    return sc.ref_library(PNG_LODEFLATE_REF)


def _on_device(bufs):
    out = [torch.from_numpy(np.array(b)).cuda() for b in bufs]
    torch.cuda.synchronize()
    return out


def _same(got, want, bufs, tile, where):
    """(sizes, HC, ZC, LD, counts) of two runs, word for word."""
    for k, what in enumerate(ARRAYS):
        assert np.array_equal(got[1 + k], want[1 + k]), (where, sc.differences(what, got[1 + k], want[1 + k], bufs, tile))
    bad = np.argwhere(got[4] != want[4])[:5]
    assert not len(bad), (where, "counts (block, word, got, want)", [(int(b), int(s), int(got[4][b, s]), int(want[4][b, s])) for b, s in bad])
    assert got[0] == want[0], where


@pytest.mark.parametrize("name", sc.CASE_IDS)
def test_device_arrays_are_the_cpu_runs(ctx, exe, tmp_path, name):
    case = sc.CASES[name]
    bufs = case.bufs()
    dev = _on_device(bufs)
    for window, tile in case.runs:
        _same(ctx.png_lodeflate_arrays(dev, window, tile), sc.cpu_run(exe, tmp_path, bufs, window, tile), bufs, tile, (name, window, tile))
    for d, b in zip(dev, bufs):
        assert np.array_equal(d.cpu().numpy(), b), "the buffer changed"


@pytest.mark.parametrize("name", sc.CASE_IDS)
def test_device_counts_are_lodepngs(ctx, ref, name):
    case = sc.CASES[name]
    bufs = case.bufs()
    dev = _on_device(bufs)
    for window, tile in case.runs:
        want_sizes, want_counts = sc.ref_run(ref, bufs, window)
        sizes, _, _, _, counts = ctx.png_lodeflate_arrays(dev, window, tile)
        bad = np.argwhere(counts != want_counts)[:5]
        assert not len(bad), (window, tile, "(block, word, got, want)", [(int(b), int(s), int(counts[b, s]), int(want_counts[b, s])) for b, s in bad])
        assert sizes == want_sizes, (window, tile)


def test_public_entry_gives_lodepngs_size_at_every_window(ctx, ref):
    seen = set()
    for name in sc.MIXTURES:
        case = sc.CASES[name]
        window = case.runs[0][0]
        seen.add(window)
        want, _ = sc.ref_run(ref, case.bufs(), window)
        assert ctx.png_deflate_sizes_device(_on_device(case.bufs()), window) == want, (name, window)
    assert seen == set(sc.WINDOWS)


def test_every_buffer_of_a_call_as_if_alone(ctx):
    """[A, A, B, A]: B's links must not reach into the tables of the A in front of it (first_tile), nor the second A's into
    the first's."""
    case = sc.CASES["same-bytes-twice"]
    bufs = case.bufs()
    dev = _on_device(bufs)
    at, blk = sc.plan_offsets(bufs)
    for window, tile in case.runs:
        sizes, hc, zc, ld, counts = ctx.png_lodeflate_arrays(dev, window, tile)
        for i, d in enumerate(dev):
            one = ctx.png_lodeflate_arrays([d], window, tile)
            part = ([sizes[i]], hc[at[i]:at[i + 1]], zc[at[i]:at[i + 1]], ld[at[i]:at[i + 1]], counts[blk[i]:blk[i + 1]])
            _same(part, one, [bufs[i]], tile, (window, tile, "buffer", i))


def test_never_seen_walks_run_beside_the_words_they_read(ctx):
    """The KEEP walks read words other lanes are resolving only while those lanes are in flight: at least 1000 positions
    whose p - W and p - 2 W are KEEPs too (the case's fact), and a launch the device holds whole, so every one of them
    runs beside the lanes of the words it reads."""
    case = sc.CASES["never-seen-256-long"]
    case.check()
    (window, tile), = case.runs
    n = len(case.bufs()[0])
    lanes = -(-n // tile) * sc.CHUNK * -(-tile // sc.CHUNK)
    props = torch.cuda.get_device_properties(0)
    assert lanes <= props.multi_processor_count * props.max_threads_per_multi_processor


_CHILD = """
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import torch
import png_lodeflate_seam_cases as sc
from zopfli_amd import Context, api
ctx = Context(0, api.library())
out = {}
for name in %r:
    case = sc.CASES[name]
    dev = [torch.from_numpy(np.array(b)).cuda() for b in case.bufs()]
    torch.cuda.synchronize()
    for window, tile in case.runs:
        sizes, hc, zc, ld, counts = ctx.png_lodeflate_arrays(dev, window, tile)
        for what, v in (("sizes", np.array(sizes)), ("HC", hc), ("ZC", zc), ("LD", ld), ("counts", counts)):
            out["%%s|%%d|%%d|%%s" %% (name, window, tile, what)] = v
ctx.close()
np.savez(%r, **out)
print("done", len(out))
"""


def test_walks_under_guard(exe, tmp_path):
    """The never-seen and zero-run cases in a fresh process under ZOPFLI_AMD_GUARD=1 (red zones around every device array,
    poisoned bodies, a check after every launch): a walk that reads outside its arrays and still lands on the right word,
    or a word no lane wrote, shows here."""
    path = str(tmp_path / "guarded.npz")
    code = _CHILD % (ROOT, os.path.join(ROOT, "tests"), GUARDED, path)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ZOPFLI_AMD_GUARD="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    got = np.load(path)
    assert r.stdout.split()[-2:] == ["done", str(len(got.files))]
    for name in GUARDED:
        case = sc.CASES[name]
        for window, tile in case.runs:
            key = f"{name}|{window}|{tile}|"
            dev = ([int(v) for v in got[key + "sizes"]],) + tuple(got[key + w] for w in ARRAYS + ("counts",))
            _same(dev, sc.cpu_run(exe, tmp_path, case.bufs(), window, tile), case.bufs(), tile, (name, window, tile))


def test_refusals_of_the_arrays_entry(ctx, gpu_lib, exe, tmp_path):
    fn = gpu_lib.zmx_internal_png_lodeflate_arrays
    fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.c_uint,
                   ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
    fn.restype = ctypes.c_int
    n = 2000
    a = sc._mixed_bytes("refusals", n)
    d, = _on_device([a])
    hc = np.full(n, 0xabababab, dtype=np.uint32)

    def call(handle, size, window, tile, out=True):
        res = (ctypes.c_uint64 * 1)(111)
        rc = fn(handle, 1, (ctypes.c_void_p * 1)(d.data_ptr()), (ctypes.c_size_t * 1)(size), window, tile, hc.ctypes.data, None, None, None,
                res if out else None)
        return rc, int(res[0])

    refused = [
        ("a tile beyond the device's", (ctx.handle, 1000, 8192, sc.DEVICE_TILE + 1)),
        ("1025 tiles of one position", (ctx.handle, 1025, 8192, 1)),
        ("2000 tiles", (ctx.handle, n, 8192, 1)),
        ("no context", (None, 1000, 8192, 0)),
        ("a size of 0", (ctx.handle, 0, 8192, 0)),
        ("window 3000", (ctx.handle, 1000, 3000, 0)),
        ("a range that leaves its allocation", (ctx.handle, 1 << 30, 8192, 0)),
    ]
    for what, args in refused:
        rc, res = call(*args)
        assert rc != 0 and gpu_lib.zmx_last_error_class() == ZMX_ERR_REFUSED, (what, gpu_lib.zmx_last_error())
        assert res == 111 and (hc == 0xabababab).all(), what
    rc, _ = call(ctx.handle, 1000, 8192, 0, out=False)
    assert rc != 0 and gpu_lib.zmx_last_error_class() == ZMX_ERR_REFUSED
    # 1024 tiles — of one position each — are taken, and the call after the refusals is right
    m = 1024
    rc, res = call(ctx.handle, m, 8192, 1)
    assert rc == 0, gpu_lib.zmx_last_error()
    want = sc.cpu_run(exe, tmp_path, [a[:m]], 8192, 1)
    assert [res] == want[0] and np.array_equal(hc[:m], want[1]) and (hc[m:] == 0xabababab).all()
    assert ctx.png_deflate_sizes_device([(d.data_ptr(), m)], 8192) == want[0]
