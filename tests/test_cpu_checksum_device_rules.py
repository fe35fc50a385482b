"""The plain-C++ rules behind zmx_checksum_device and the PNG left in device memory, on the CPU, through
tests/hostlib/checksum_device_print.cc: the piece split from a range's end, the device's combine and finish
(device/zmx_checksum_device.h) against zlib, at the lengths around a lane and a piece; the frame's literals
(host/device_output_plan.h) against the container written in Python and against PngAssemble; zmx_png_bound's arithmetic
against an all-stored stream.  The program is built a second time with sanitizers and run on its own."""
import functools
import os
import subprocess
import zlib

import numpy as np
import pytest

import png_encode_cases as ec
from zopfli_amd._build import ROOT

HOSTLIB_DIR = os.path.join(ROOT, "tests", "hostlib")
BUILD = os.path.join(ROOT, "tests", "_build")
PIECE = 262144
LENGTHS = [0, 1, 3, 4, 5, 1023, 1024, 1025, PIECE - 1, PIECE, PIECE + 1, 2 * PIECE + 5]
FILLS = ["zeros", "ones", "random"]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request):
    if request.param == "plain":
        subprocess.check_call(["make", "-s", "-C", HOSTLIB_DIR, "-f", "checksum_device.mk"])
        return os.path.join(BUILD, "checksum_device_print")
    subprocess.check_call(["make", "-s", "-C", HOSTLIB_DIR, "-f", "checksum_device.mk", "SANITIZE=-fsanitize=address,undefined", "SUFFIX=_san"])
    return os.path.join(BUILD, "checksum_device_print_san")


@functools.lru_cache(maxsize=None)
def _random_bytes(n):
    """checksum_device_print.cc's Fill("random"): a 32-bit linear congruential generator seeded with the length, its top byte."""
    out = np.empty(n, dtype=np.uint8)
    x = (n * 2654435761 + 12345) & 0xffffffff
    for i in range(n):
        x = (x * 1664525 + 1013904223) & 0xffffffff
        out[i] = x >> 24
    return out.tobytes()


def _bytes(fill, n):
    return b"\x00" * n if fill == "zeros" else b"\xff" * n if fill == "ones" else _random_bytes(n)


def test_pieces_combine_and_finish_against_zlib(exe):
    cases = [(fill, n, shift) for fill in FILLS for n in LENGTHS for shift in ((0, 1, 3) if n in (0, 5, 1025, PIECE + 1) else (n % 4,))]
    r = subprocess.run([exe, "sums"], input="".join(f"{f} {n} {s}\n" for f, n, s in cases), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    for (fill, n, shift), line in zip(cases, lines):
        npieces, crc, adler, sealed, begin = line.split()
        data = _bytes(fill, n)
        want_crc = zlib.crc32(data) & 0xffffffff
        assert int(npieces) == (n + PIECE - 1) // PIECE, (fill, n, shift)
        assert int(crc) == want_crc, (fill, n, shift)
        assert int(adler) == zlib.adler32(data) & 0xffffffff, (fill, n, shift)
        assert sealed == "%08x" % want_crc, (fill, n, shift)   # most significant byte first
        assert int(begin) == shift, (fill, n, shift)


@pytest.fixture(scope="module")
def container_exe():
    subprocess.check_call(["make", "-s", "-C", HOSTLIB_DIR, "-f", "png_rows.mk"])
    return os.path.join(BUILD, "png_container_print")


@pytest.mark.parametrize("shape", ec.SHAPES[:4] + [ec.WIDE], ids=ec.shape_id)
def test_frame_literals_make_the_container(exe, container_exe, tmp_path, shape):
    """The frame's header, a zlib stream's body and Adler-32, the frame's tail with zlib.crc32 in the placeholder: the file
    png_encode_cases.assemble writes, and the one PngAssemble makes."""
    raw = b"".join(b"\x02" + bytes(r) for r in ec.pixels(shape))
    stream = zlib.compress(raw, 9)
    assert stream[:2] == b"\x78\xda"
    r = subprocess.run([exe, "frame"] + [str(v) for v in shape] + [str(len(stream))], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    header, tail = (bytes.fromhex(h) for h in r.stdout.split())
    assert len(header) == 41 + 2 and header[-2:] == b"\x78\x01" and len(tail) == 16 and tail[:4] == b"\x00" * 4
    payload = header[-2:] + stream[2:]
    crc = zlib.crc32(header[-6:-2] + payload) & 0xffffffff   # "IDAT" and the payload: what the device seals
    made = header[:-2] + payload + crc.to_bytes(4, "big") + tail[4:]
    assert made == ec.assemble(shape, stream)
    assert [t for t, _ in ec.chunks(made)] == [b"IHDR", b"IDAT", b"IEND"]
    src, dst = str(tmp_path / "stream.bin"), str(tmp_path / "made.png")
    with open(src, "wb") as f:
        f.write(stream)
    r = subprocess.run([container_exe, src, dst] + [str(v) for v in shape], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr[-1000:])
    with open(dst, "rb") as f:
        assert made == f.read()


def test_frame_refuses_a_stream_beyond_a_chunks_length(exe):
    ok = subprocess.run([exe, "frame", "1", "1", "0", "8", str(0x7fffffff)], capture_output=True, text=True)
    assert ok.returncode == 0 and bytes.fromhex(ok.stdout.split()[0])[33:37] == b"\x7f\xff\xff\xff"
    r = subprocess.run([exe, "frame", "1", "1", "0", "8", str(0x80000000)], capture_output=True, text=True)
    assert r.returncode == 1 and r.stdout.split() == ["refused"]


def _all_stored_file(scanlines):
    """The PNG around a zlib stream whose every master block (1 000 000 bytes) is stored in pieces of at most 65535 bytes,
    each with its five bytes of header, LEN and NLEN: the largest file AddLZ77BlockAutoType's fallback allows."""
    stream = 2 + 4
    for start in range(0, max(scanlines, 1), 1000000):
        m = min(1000000, scanlines - start)
        stream += m + 5 * max(1, (m + 65534) // 65535)
    return 41 + stream + 16


@pytest.mark.parametrize("width,height", [(65533, 1), (65534, 1), (65535, 1), (65536, 1), (131069, 1), (131070, 1), (999, 1000), (999, 1001),
                                          (1000, 999), (1999, 1000), (1999, 1001), (1, 1), (1, 32768), (1, 500001)])
def test_bound_covers_an_all_stored_stream(exe, width, height):
    r = subprocess.run([exe, "bound", str(width), str(height), "0", "8"], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    bound, scanlines = (int(v) for v in r.stdout.split())
    assert scanlines == height * (width + 1)
    assert bound >= _all_stored_file(scanlines), (bound, _all_stored_file(scanlines))
