"""The container of zmx_png_encode_device (zopfli_amd/csrc/host/png_container.h) on the CPU, through
tests/hostlib/png_container_print.cc: around the IDAT payload of a file the reference's zopflipng wrote — its second byte
set back to zopfli's own DA — it must give that file back byte for byte, for the four colour types at both depths; and
the same from a stream zlib made, against the container written in Python."""
import os
import subprocess
import zlib

import pytest

import png_encode_cases as ec
from png_rows_cases import filter_rows
from zopfli_amd._build import PNG_REF, ROOT

HOSTLIB_DIR = os.path.join(ROOT, "tests", "hostlib")
BUILD = os.path.join(ROOT, "tests", "_build")


@pytest.fixture(scope="module")
def exe():
    subprocess.check_call(["make", "-s", "-C", HOSTLIB_DIR, "-f", "png_rows.mk"])
    return os.path.join(BUILD, "png_container_print")


def _container(exe, tmp_path, shape, stream, expect_ok=True, piece=None):
    src, dst = str(tmp_path / "stream.bin"), str(tmp_path / "made.png")
    with open(src, "wb") as f:
        f.write(stream)
    r = subprocess.run([exe, src, dst] + [str(v) for v in shape] + ([str(piece)] if piece else []), capture_output=True, text=True)
    if not expect_ok:
        assert r.returncode == 1 and r.stdout.split() == ["refused"], (r.stdout, r.stderr[-1000:])
        return None
    assert r.returncode == 0, (r.stdout, r.stderr[-1000:])
    with open(dst, "rb") as f:
        png = f.read()
    bw = ec.bytewidth(shape)
    assert r.stdout.split() == ["ok", str(len(png)), str(bw), str(shape[0] * bw)]
    return png


@pytest.mark.parametrize("shape", ec.SHAPES, ids=ec.shape_id)
def test_container_gives_the_references_file_back(exe, tmp_path, shape):
    if not os.path.exists(PNG_REF):
        pytest.skip("oracle/_ref/zopflipng_ref not built (needs the reference's sources at build time)")
    src, ref = str(tmp_path / "in.png"), str(tmp_path / "ref.png")
    with open(src, "wb") as f:
        img = ec.pixels(shape)
        f.write(ec.plain_png(shape, filter_rows(img, ec.bytewidth(shape), ec.mixed_types(shape[1]))))
    r = subprocess.run([PNG_REF, "-y", "--always_zopflify", "--keepcolortype", "--iterations=1", src, ref],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-1000:])
    with open(ref, "rb") as f:
        want = f.read()
    parts = ec.chunks(want)
    assert [t for t, _ in parts] == [b"IHDR", b"IDAT", b"IEND"]
    payload = parts[1][1]
    assert payload[:2] == b"\x78\x01"
    assert _container(exe, tmp_path, shape, b"\x78\xda" + payload[2:]) == want


@pytest.mark.parametrize("shape", ec.SHAPES[:4], ids=ec.shape_id)
def test_container_vs_python(exe, tmp_path, shape):
    """No reference at hand: a level-9 zlib stream begins 78 DA as zopfli's does; the file is the one written in Python,
    and it decodes to the scanlines."""
    img = ec.pixels(shape)
    raw = b"".join(b"\x02" + bytes(r) for r in img)
    stream = zlib.compress(raw, 9)
    assert stream[:2] == b"\x78\xda"
    png = _container(exe, tmp_path, shape, stream)
    assert png == ec.assemble(shape, stream)
    assert zlib.decompress(ec.chunks(png)[1][1]) == raw
    # the IDAT's CRC-32 in pieces on threads: any share gives the same file
    for piece in (1, 7, len(stream) // 3, len(stream) // 2):
        assert _container(exe, tmp_path, shape, stream, piece=piece) == png, piece


def test_sanitized_container(tmp_path):
    """The same program under AddressSanitizer and UBSan (host code, its own main), threads included."""
    subprocess.check_call(["make", "-s", "-C", HOSTLIB_DIR, "-f", "png_rows.mk", "SANITIZE=-fsanitize=address,undefined", "SUFFIX=_san"])
    san = os.path.join(BUILD, "png_container_print_san")
    shape = ec.SHAPES[1]
    stream = zlib.compress(b"".join(b"\x01" + bytes(r) for r in ec.pixels(shape)), 9)
    for piece in (None, 5, 100):
        assert _container(san, tmp_path, shape, stream, piece=piece) == ec.assemble(shape, stream)


def test_container_refuses(exe, tmp_path):
    """What is no zopfli zlib stream, and formats the entry does not take."""
    good = zlib.compress(b"\x00abc", 9)
    _container(exe, tmp_path, (3, 1, 0, 8), b"\x78\x9c" + good[2:], expect_ok=False)
    _container(exe, tmp_path, (3, 1, 0, 8), good[:5], expect_ok=False)
    _container(exe, tmp_path, (3, 1, 3, 8), good, expect_ok=False)      # palette
    _container(exe, tmp_path, (3, 1, 0, 4), good, expect_ok=False)      # four bits
    assert _container(exe, tmp_path, (3, 1, 0, 8), good) is not None
