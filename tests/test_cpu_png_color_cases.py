"""Colour-type reduction on the CPU.  The numpy model of tests/png_color_cases.py is held against the all-reference
zopflipng (oracle/_ref/zopflipng_ref, strategy 0, 2 iterations) on every case: IHDR, PLTE, tRNS and the inflated IDAT,
and the whole file where zopflipng makes its second try.  The rules of zopfli_amd/csrc/device/zmx_png_color.h and
zopfli_amd/csrc/host/png_color_choose.h are run by tests/hostlib/png_color_print.cc, the threads of a launch one after
the other, and must give the model's statistics, mode and converted bytes at every alignment of the destination, leave
the guard bytes around the output and the image as they were; the same program is run under AddressSanitizer and
UBSan.  The container's prefix with PLTE and tRNS is held against struct and zlib.crc32."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import oracle_lib as ol
import png_color_cases as cc
import png_encode_cases as ec
from png_rows_cases import filter_rows
from zopfli_amd._build import PNG_REF, ROOT

HOSTLIB_DIR = os.path.join(ROOT, "tests", "hostlib")
BUILD = os.path.join(ROOT, "tests", "_build")
ITERATIONS = 2


def _make(*extra):
    subprocess.check_call(["make", "-s", "-C", HOSTLIB_DIR, "-f", "png_color.mk", *extra])


@pytest.fixture(scope="module")
def exe():
    _make()
    return os.path.join(BUILD, "png_color_print")


def _run(exe, tmp_path, case, src_mod, dst_mod, which="auto"):
    """png_color_print on a case: (statistics, mode, converted bytes) in the model's terms."""
    name, w, h, ct, depth = case
    src, out = os.path.join(str(tmp_path), "in.bin"), os.path.join(str(tmp_path), "out.bin")
    with open(src, "wb") as f:
        f.write(cc.pixels(case).tobytes())
    r = subprocess.run([exe, src, out, str(src_mod), str(dst_mod), str(w), str(h), str(ct), str(depth), which], capture_output=True, text=True)
    assert r.returncode == 0, (name, r.stdout, r.stderr[-2000:])
    parts = [p.split() for p in r.stdout.split("|")]
    assert parts[0][0] == "ok", r.stdout
    s = [int(x) for x in parts[0][1:]]
    m = [int(x) for x in parts[1]]
    g = [int(x) for x in parts[2]]
    hexpal = parts[3][0]
    palette = np.zeros((0, 4), dtype=np.uint8) if hexpal == "-" else np.frombuffer(bytes.fromhex(hexpal), dtype=np.uint8).reshape(-1, 4)
    st = {"colored": bool(s[0]), "key": bool(s[1]), "alpha": bool(s[2]), "numcolors": s[3], "bits": s[4], "key_rgb": tuple(s[5:8]),
          "palette": palette}
    mode = {"colortype": m[0], "bitdepth": m[1], "palette": palette[:m[2]] if m[0] == 3 else None, "key": tuple(m[4:7]) if m[3] else None}
    assert m[2] == (len(palette) if m[0] == 3 else 0)
    assert g[0] == cc.rowbytes(w, mode) and g[3] == -1, r.stdout
    assert 1 <= g[1] <= 2048 and 1 <= g[2] <= 2048
    return st, mode, np.fromfile(out, dtype=np.uint8).reshape(h, g[0])


def _same_stats(a, b):
    return all(a[k] == b[k] for k in ("colored", "key", "alpha", "numcolors", "bits", "key_rgb")) and np.array_equal(a["palette"], b["palette"])


def _same_mode(a, b):
    if (a["colortype"], a["bitdepth"], a["key"]) != (b["colortype"], b["bitdepth"], b["key"]):
        return False
    return a["palette"] is None and b["palette"] is None or np.array_equal(a["palette"], b["palette"])


def _mods(name):
    k = zlib.crc32(name.encode())
    return (k >> 4) % 16, (k >> 8) % 16


def _reference(tmp_path, case, letter="0"):
    """The all-reference zopflipng's file for a PNG of the case's pixels in their own colour type."""
    name, w, h, ct, depth = case
    src, dst = str(tmp_path / "in.png"), str(tmp_path / "ref.png")
    img = cc.pixels(case)
    bw = ec.CHANNELS[ct] * depth // 8
    with open(src, "wb") as f:
        f.write(ec.plain_png((w, h, ct, depth), filter_rows(img, bw, np.zeros(h, dtype=np.uint8))))
    r = subprocess.run([PNG_REF, "-y", "--always_zopflify", f"--iterations={ITERATIONS}", f"--filters={letter}", src, dst],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-1000:])
    with open(dst, "rb") as f:
        return f.read()


def _model_file(case, mode):
    """The file of the case in `mode` under strategy 0, deflated by the reference's library."""
    name, w, h, ct, depth = case
    rgba = cc.model(case)[0]
    conv = cc.convert(rgba, depth, w, h, mode)
    scan = filter_rows(conv, cc.bytewidth(mode), np.zeros(h, dtype=np.uint8))
    return cc.assemble(w, h, mode, ol.ref_compress(scan.tobytes(), 1, ITERATIONS))


@pytest.mark.parametrize("case", cc.CASES, ids=cc.IDS)
def test_model_is_zopflipngs(tmp_path, case):
    if not os.path.exists(PNG_REF) or not ol.have_ref():
        pytest.skip("oracle/_ref/zopflipng_ref not built (needs the reference's sources at build time)")
    name, w, h, ct, depth = case
    rgba, st, mode, conv = cc.model(case)
    ref = _reference(tmp_path, case)
    first = _model_file(case, mode)
    retried = None
    if mode["colortype"] == 3 and len(first) < cc.RETRY_BELOW:
        second = _model_file(case, cc.retry_mode(st, w * h))
        retried = len(second) < len(first)
        if retried:
            first, mode = second, cc.retry_mode(st, w * h)
    # chunk by chunk first, so that a difference says where it is
    got = dict(ec.chunks(ref))
    assert [t for t, _ in ec.chunks(ref)] == cc.expected_chunks(mode), name
    assert got[b"IHDR"] == cc.ihdr(w, h, mode)[8:-4]
    want = dict(ec.chunks(first))
    assert got.get(b"PLTE") == want.get(b"PLTE") and got.get(b"tRNS") == want.get(b"tRNS"), name
    conv = cc.convert(rgba, depth, w, h, mode)
    assert zlib.decompress(got[b"IDAT"]) == filter_rows(conv, cc.bytewidth(mode), np.zeros(h, dtype=np.uint8)).tobytes(), name
    assert ref == first, name
    reached = cc.model(case)[2]
    assert cc.EXPECT[name] == (reached["colortype"], reached["bitdepth"], 0 if reached["palette"] is None else len(reached["palette"]),
                               reached["key"], retried), name


@pytest.mark.parametrize("case", cc.CASES, ids=cc.IDS)
def test_model_reaches_what_the_case_is_for(case):
    """Without the reference: the mode and the palette size of the table."""
    name, w, h, ct, depth = case
    mode = cc.model(case)[2]
    assert cc.EXPECT[name][:4] == (mode["colortype"], mode["bitdepth"], 0 if mode["palette"] is None else len(mode["palette"]), mode["key"])
    # the cases whose mode is the image's own: nothing is converted for them
    assert cc.same_mode(ct, depth, mode) == (name in cc.AS_IS), name


@pytest.mark.parametrize("case", cc.CASES, ids=cc.IDS)
def test_rules(exe, tmp_path, case):
    rgba, st, mode, conv = cc.model(case)
    src_mod, dst_mod = _mods(case[0])
    got_st, got_mode, got = _run(exe, tmp_path, case, src_mod, dst_mod)
    assert _same_stats(got_st, st), (case[0], got_st, st)
    assert _same_mode(got_mode, mode), (case[0], got_mode, mode)
    assert np.array_equal(got, conv), case[0]
    if mode["colortype"] == 3:
        name, w, h, ct, depth = case
        want_mode = cc.retry_mode(st, w * h)
        _, got_mode, got = _run(exe, tmp_path, case, src_mod, dst_mod, "retry")
        assert _same_mode(got_mode, want_mode), case[0]
        assert np.array_equal(got, cc.convert(rgba, depth, w, h, want_mode)), case[0]


@pytest.mark.parametrize("name", ["colors-5", "colors-17", "grey1-w9-ct6", "grey2-w37-ct6", "grey4-w7-ct0", "colors-3", "fake16", "true16-grey",
                                  "true16-rgb-key", "grey-alpha"])
def test_every_offset(exe, tmp_path, name):
    """Every address of the output mod 16, the image moving the other way; the workgroups in both orders."""
    case = cc.CASES[cc.IDS.index(name)]
    rgba, st, mode, conv = cc.model(case)
    for dst_mod in range(16):
        got_st, got_mode, got = _run(exe, tmp_path, case, (7 * dst_mod + 3) % 16, dst_mod)
        assert _same_stats(got_st, st) and _same_mode(got_mode, mode), (name, dst_mod)
        assert np.array_equal(got, conv), (name, dst_mod)


def test_sanitized_program(tmp_path):
    """The same program under AddressSanitizer and UBSan (host code, its own main): the image lies in a heap block that
    ends with its last byte, so a read beyond it is reported."""
    _make("SANITIZE=-fsanitize=address,undefined", "SUFFIX=_san")
    san = os.path.join(BUILD, "png_color_print_san")
    for case in cc.CASES:
        rgba, st, mode, conv = cc.model(case)
        src_mod, dst_mod = _mods(case[0] + "san")
        got_st, got_mode, got = _run(san, tmp_path, case, src_mod, dst_mod)
        assert _same_stats(got_st, st) and _same_mode(got_mode, mode) and np.array_equal(got, conv), case[0]


def _prefix_file(exe, tmp_path, w, h, mode, stream):
    src, out = str(tmp_path / "z.bin"), str(tmp_path / "out.png")
    with open(src, "wb") as f:
        f.write(stream)
    pal = "-" if mode["palette"] is None else np.asarray(mode["palette"], dtype=np.uint8).tobytes().hex()
    key = mode["key"] or (0, 0, 0)
    r = subprocess.run([exe, src, out, str(w), str(h), str(mode["colortype"]), str(mode["bitdepth"]), pal, str(int(mode["key"] is not None)),
                        *[str(k) for k in key]], capture_output=True, text=True)
    if r.returncode != 0:
        return None
    with open(out, "rb") as f:
        return f.read()


def test_container_prefix(tmp_path):
    """PLTE, tRNS, colour type 3 and the depths below 8 against struct and zlib.crc32; what PNG has not is refused."""
    _make()
    exe = os.path.join(BUILD, "png_prefix_print")
    stream = b"\x78\xda" + zlib.compress(b"scanlines" * 50, 9)[2:]
    opaque = np.array([(1, 2, 3, 255), (4, 5, 6, 255)], dtype=np.uint8)
    some = np.array([(1, 2, 3, 255), (4, 5, 6, 0), (7, 8, 9, 255), (9, 9, 9, 255)], dtype=np.uint8)
    full = np.array([(i, 255 - i, i ^ 85, (i * 7) & 255) for i in range(256)], dtype=np.uint8)
    full[255, 3] = 1
    modes = [
        {"colortype": 3, "bitdepth": 1, "palette": opaque, "key": None},
        {"colortype": 3, "bitdepth": 2, "palette": some, "key": None},
        {"colortype": 3, "bitdepth": 4, "palette": some[:3], "key": None},
        {"colortype": 3, "bitdepth": 8, "palette": full, "key": None},
        {"colortype": 0, "bitdepth": 1, "palette": None, "key": None},
        {"colortype": 0, "bitdepth": 2, "palette": None, "key": (1, 1, 1)},
        {"colortype": 0, "bitdepth": 16, "palette": None, "key": (0xabcd, 0xabcd, 0xabcd)},
        {"colortype": 2, "bitdepth": 8, "palette": None, "key": (1, 2, 3)},
        {"colortype": 2, "bitdepth": 16, "palette": None, "key": (0x0102, 0x0304, 0x0506)},
        {"colortype": 6, "bitdepth": 8, "palette": None, "key": None},
        {"colortype": 4, "bitdepth": 16, "palette": None, "key": None},
    ]
    for mode in modes:
        got = _prefix_file(exe, tmp_path, 300, 7, mode, stream)
        assert got == cc.assemble(300, 7, mode, stream), mode
        assert [t for t, _ in ec.chunks(got)] == cc.expected_chunks(mode)
    for ct, depth in ((3, 16), (2, 4), (6, 1), (1, 8), (0, 3), (4, 4)):
        assert _prefix_file(exe, tmp_path, 3, 3, {"colortype": ct, "bitdepth": depth, "palette": None, "key": None}, stream) is None
    # a stream that is none is refused as PngClose refuses it
    assert _prefix_file(exe, tmp_path, 3, 3, modes[0], b"\x78\x9c" + stream[2:]) is None
