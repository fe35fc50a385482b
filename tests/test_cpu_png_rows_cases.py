"""The filtered scanlines of zmx_png_filter_rows_device on the CPU.  The numpy reference of tests/png_rows_cases.py is
held against LodePNG's own filter (oracle/_ref/libpng_filter_ref.so, strategies LFS_ZERO .. LFS_FOUR) on every image of
the table; the rules of zopfli_amd/csrc/device/zmx_png_rows.h — the mapping from an output byte to (row, x), the
byte-wise filters, the in-row vectors — are run by tests/hostlib/png_rows_print.cc, the threads of the launch one after
the other, and must give the reference's bytes, leave the guard bytes around the output and the image as they were and
read nothing outside the image's aligned words; the same program is run under AddressSanitizer and UBSan."""
import ctypes
import os
import subprocess
import zlib

import numpy as np
import pytest

import png_rows_cases as pc
from zopfli_amd._build import PNG_FILTER_REF, ROOT

HOSTLIB_DIR = os.path.join(ROOT, "tests", "hostlib")
BUILD = os.path.join(ROOT, "tests", "_build")
IDS = [c[0] for c in pc.TABLE]


def _make(*extra):
    subprocess.check_call(["make", "-s", "-C", HOSTLIB_DIR, "-f", "png_rows.mk", *extra])


def _run(exe, tmp_path, img, types, bytewidth, src_mod, dst_mod):
    src = os.path.join(str(tmp_path), "in.bin")
    out = os.path.join(str(tmp_path), "out.bin")
    h, n = img.shape
    with open(src, "wb") as f:
        f.write(img.tobytes() + np.asarray(types, dtype=np.uint8).tobytes())
    r = subprocess.run([exe, src, out, str(src_mod), str(dst_mod), str(n), str(h), str(bytewidth)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    words = r.stdout.split()
    total = h * (n + 1)
    assert words[:3] == ["ok", str(total), str(pc.grid(total))]
    return np.fromfile(out, dtype=np.uint8).reshape(h, n + 1), int(words[3])


@pytest.fixture(scope="module")
def exe():
    _make()
    return os.path.join(BUILD, "png_rows_print")


@pytest.fixture(scope="module")
def lodepng():
    if not os.path.exists(PNG_FILTER_REF):
        pytest.skip("oracle/_ref/libpng_filter_ref.so not built (needs the reference's sources at build time)")
    lib = ctypes.CDLL(PNG_FILTER_REF)
    lib.ref_png_filter.argtypes = [ctypes.c_char_p, ctypes.c_char_p] + [ctypes.c_uint] * 5
    lib.ref_png_filter.restype = ctypes.c_uint
    return lib


@pytest.mark.parametrize("case", pc.TABLE, ids=IDS)
def test_reference_is_lodepngs(lodepng, case):
    """filter_rows with one type for all rows == LodePNG's filter() under LFS_ZERO .. LFS_FOUR (lodepng.h: 0 .. 4)."""
    _, n, h, bw, _, _ = case
    img, _ = pc.make(case)
    colortype, depth = pc.LODEPNG_MODE[bw]
    assert n % bw == 0
    for t in range(5):
        out = ctypes.create_string_buffer(h * (n + 1))
        assert lodepng.ref_png_filter(out, img.tobytes(), n // bw, h, colortype, depth, t) == 0
        got = np.frombuffer(out.raw, dtype=np.uint8).reshape(h, n + 1)
        assert np.array_equal(got, pc.filter_rows(img, bw, np.full(h, t, dtype=np.uint8))), (case[0], t)


def _mods(name):
    k = zlib.crc32(name.encode())
    return (k >> 4) % 16, (k >> 8) % 16


@pytest.mark.parametrize("case", pc.TABLE + [pc.BIG], ids=IDS + [pc.BIG[0]])
def test_rules(exe, tmp_path, case):
    img, types = pc.make(case)
    src_mod, dst_mod = _mods(case[0])
    got, bad = _run(exe, tmp_path, img, types, case[3], src_mod, dst_mod)
    assert bad == -1
    assert np.array_equal(got, pc.filter_rows(img, case[3], types)), case[0]


@pytest.mark.parametrize("name", ["short-5", "short-17", "short-36", "long-65-bw1", "long-1024-bw4", "width-1-bw8"])
def test_every_offset(exe, tmp_path, name):
    """Every address of the output mod 16, the image moving the other way."""
    case = pc.TABLE[IDS.index(name)]
    img, types = pc.make(case)
    want = pc.filter_rows(img, case[3], types)
    for dst_mod in range(16):
        got, _ = _run(exe, tmp_path, img, types, case[3], (7 * dst_mod + 3) % 16, dst_mod)
        assert np.array_equal(got, want), (name, dst_mod)


def test_bad_type_is_reported(exe, tmp_path):
    """A type byte above 4 is reported with its row (the first of them), copied into the output, and its row left
    unfiltered; the other rows are as ever."""
    case = pc.TABLE[IDS.index("gradient")]
    img, types = pc.make(case)
    types = types.copy()
    types[[11, 29]] = [5, 200]
    got, bad = _run(exe, tmp_path, img, types, case[3], 0, 9)
    assert bad == 11
    ok = types <= 4
    want = pc.filter_rows(img, case[3], np.where(ok, types, 0))
    assert np.array_equal(got[:, 1:], want[:, 1:]) and np.array_equal(got[:, 0], types)


def test_sanitized_program(tmp_path):
    """The same program under AddressSanitizer and UBSan (host code, its own main): the image lies in a heap block that
    ends with the last aligned word holding one of its bytes, so a read beyond what the header promises is reported."""
    _make("SANITIZE=-fsanitize=address,undefined", "SUFFIX=_san")
    san = os.path.join(BUILD, "png_rows_print_san")
    for case in pc.TABLE:
        img, types = pc.make(case)
        src_mod, dst_mod = _mods(case[0] + "san")
        got, _ = _run(san, tmp_path, img, types, case[3], src_mod, dst_mod)
        assert np.array_equal(got, pc.filter_rows(img, case[3], types)), case[0]
