"""--lossy_transparent and --lossy_8bit on the CPU.  The numpy model of tests/png_lossy_cases.py is held against the
all-reference zopflipng (oracle/_ref/zopflipng_ref, --keepcolortype --filters=0: the inflated IDAT; for the entries' cases
the whole file without --keepcolortype, and the --lossy_8bit combinations).  The rules of
zopfli_amd/csrc/device/zmx_png_lossy.h are run by tests/hostlib/png_lossy_print.cc, the threads of a launch one after the
other, and must give the model's info and image at every alignment, out of place and in place, the workgroups in both
orders, and leave the guard bytes around the output and the image as they were; the same program is run under
AddressSanitizer and UBSan.  The cases tell mistaken variants of the model from the right one."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import oracle_lib as ol
import png_color_cases as cc
import png_encode_cases as ec
import png_lossy_cases as lc
from png_rows_cases import filter_rows
from zopfli_amd._build import PNG_REF, ROOT

HOSTLIB_DIR = os.path.join(ROOT, "tests", "hostlib")
BUILD = os.path.join(ROOT, "tests", "_build")
ITERATIONS = 2


def _make(*extra):
    subprocess.check_call(["make", "-s", "-C", HOSTLIB_DIR, "-f", "png_lossy.mk", *extra])


@pytest.fixture(scope="module")
def exe():
    _make()
    return os.path.join(BUILD, "png_lossy_print")


def _run(exe, tmp_path, case, src_mod, dst_mod, inplace=False):
    """png_lossy_print on a case: (info in the model's terms, rewritten image, geometry)."""
    name, w, h, ct, depth = case
    src, out = os.path.join(str(tmp_path), "in.bin"), os.path.join(str(tmp_path), "out.bin")
    with open(src, "wb") as f:
        f.write(lc.pixels(case).tobytes())
    r = subprocess.run([exe, src, out, str(src_mod), str(dst_mod), str(w), str(h), str(ct), str(depth), "inplace" if inplace else "out"],
                       capture_output=True, text=True)
    assert r.returncode == 0, (name, r.stdout, r.stderr[-2000:])
    parts = [p.split() for p in r.stdout.split("|")]
    assert parts[0][0] == "ok", r.stdout
    s = [int(x) for x in parts[0][1:]]
    info = {"mode": s[0], "partial_alpha": s[1], "numcolors": s[2], "fill": tuple(s[3:6]), "first_transparent": None if s[6] < 0 else s[6]}
    return info, np.fromfile(out, dtype=np.uint8).reshape(h, -1), [int(x) for x in parts[1]]


def _mods(name):
    k = zlib.crc32(name.encode())
    return (k >> 4) % 16, (k >> 8) % 16


def _check(got, case, what):
    info, img, geometry = got
    want_info, want = lc.model(case)
    assert info == want_info, (case[0], what, info, want_info)
    assert np.array_equal(img, want), (case[0], what)
    assert 1 <= geometry[4] <= lc.MAX_GROUPS


def test_geometry_is_the_headers(exe, tmp_path):
    """The names of png_lossy_cases are the header's: a chunk, a tile, a sweep, the scan's step, the grid's cap."""
    for name in ("run-tiles", "ga-carry", "rgba16-hi", "ga16-hi"):
        case = lc.case(name)
        _, w, h, ct, depth = case
        g = _run(exe, tmp_path, case, 0, 0)[2]
        tiles = -(-w * h // lc.tile_pixels(ct, depth))
        assert g == [lc.chunk_pixels(ct, depth), lc.tile_pixels(ct, depth), lc.sweep_pixels(ct, depth), lc.SCAN_STEP, min(tiles, lc.MAX_GROUPS), tiles]
    assert (lc.C, lc.W, lc.T, lc.SWEEP) == (12, 768, 3072, 2048 * 3072)
    # the large cases are what they are for: more tiles than a step of the scan, more pixels than a sweep
    _, w, h, ct, depth = lc.case("run-scan-step")
    assert w * h > (lc.SCAN_STEP + 2) * lc.tile_pixels(ct, depth)
    _, w, h, ct, depth = lc.case("run-sweep")
    assert lc.sweep_pixels(ct, depth) + lc.tile_pixels(ct, depth) < w * h < 2 * lc.sweep_pixels(ct, depth)


@pytest.mark.parametrize("case", lc.CASES, ids=lc.IDS)
def test_model_reaches_what_the_case_is_for(case):
    name, w, h, ct, depth = case
    info, out = lc.model(case)
    assert lc.EXPECT[name] == (info["mode"], info["partial_alpha"] == 0, info["numcolors"] <= 256, info["first_transparent"]), name
    v, r = lc.view8(lc.pixels(case), w, h, ct, depth), lc.view8(out, w, h, ct, depth)
    a = v[:, 3]
    assert np.array_equal(r[:, 3], a) and np.array_equal(r[a > 0], v[a > 0]), "alpha and the pixels with a > 0 stay"
    if depth == 16:
        assert np.array_equal(np.asarray(out).reshape(-1, 2)[:, 1], lc.pixels(case).reshape(-1, 2)[:, 1]), "the low bytes stay"
    if info["mode"] == lc.MODE_CARRY:
        assert np.any(a > 0), "an image without an opaque pixel has no partial alpha: it cannot be carry mode"
    if name == "all-transparent":
        assert info["mode"] == lc.MODE_FIXED and np.all(r[:, :3] == v[0, :3])
    if name == "carry-leading":
        assert np.all(r[:5, :3] == 0) and np.any(v[:5, :3] != 0)
    if name == "idempotent":
        assert np.array_equal(out, lc.pixels(case)) and not np.array_equal(out, lc.pixels(lc.case("stays-rgba")))
    if name in lc.ENTRY_CASES:
        got = []
        for flags in range(4):
            img, d = lc.prepared(case, flags, True)
            got.append(lc.mode_tuple(lc.reduced(img, w, h, ct, d)[2]))
        assert got == lc.OPTIMIZE_EXPECT[name], name


def test_carry_passes_through_empty_tiles():
    """run-tiles: two whole tiles without an opaque pixel; run-scan-step: the run crosses a step of the scan; run-sweep: the
    sweep of a full launch."""
    for name, lo, hi in (("run-tiles", 1, 3), ("run-scan-step", lc.SCAN_STEP - 1, lc.SCAN_STEP + 2), ("run-sweep", lc.MAX_GROUPS - 1, lc.MAX_GROUPS + 1)):
        _, w, h, ct, depth = case = lc.case(name)
        a = lc.view8(lc.pixels(case), w, h, ct, depth)[:, 3]
        t = lc.tile_pixels(ct, depth)
        assert not np.any(a[lo * t:hi * t]) and np.any(a[max(lo - 2, 0) * t:lo * t]) and np.any(a[hi * t:(hi + 1) * t]), name
    for name, last, first in (("tile-end-opaque", True, False), ("tile-end-transparent", False, True)):
        _, w, h, ct, depth = case = lc.case(name)
        a = lc.view8(lc.pixels(case), w, h, ct, depth)[:, 3]
        assert (a[lc.T - 1] != 0, a[lc.T] != 0) == (last, first), name


# which cases tell a mistaken variant from the right rule (at least these)
TELLS = {
    "carry-resets-at-row": ["run-row-end", "w1-column", "ga-carry"],
    "carry-resets-at-tile": ["run-tile", "run-tiles", "tile-end-opaque", "run-scan-step"],
    "last-transparent": ["first-at-0", "first-at-tile", "buys-key"],
    "partial-includes-0": ["first-at-chunk", "buys-key", "fake16-key"],
    "partial-below-254": ["alpha-254-last"],
    "partial-above-1": ["alpha-1-last"],
    "transparent-by-rgb": ["many-transparent-rgbs", "pal-255-and-transparent", "zero-beside", "buys-palette"],
    "threshold-255": ["pal-255-and-transparent"],
    "threshold-257": ["pal-256-and-transparent", "257th-last-tile"],
    "carry-despite-palette": ["many-transparent-rgbs", "pal-255-and-transparent"],
    "fixed-always": ["run-chunk", "stays-rgba", "257th-last-tile"],
    "alpha-touched": ["one-transparent", "run-wave"],
    "opaque-touched": ["run-wave", "first-at-wave"],
}


@pytest.mark.parametrize("wrong", lc.WRONG)
def test_cases_tell_wrong_variants(wrong):
    assert set(TELLS) == set(lc.WRONG)
    for name in TELLS[wrong]:
        _, w, h, ct, depth = case = lc.case(name)
        assert not np.array_equal(lc.lossy_transparent(lc.pixels(case), w, h, ct, depth, wrong=wrong)[1], lc.model(case)[1]), (wrong, name)


def test_cases_tell_the_low_byte():
    for name in ("rgba16-hi", "ga16-hi"):
        _, w, h, ct, depth = case = lc.case(name)
        assert not np.array_equal(lc.to_8bit(lc.pixels(case), w, h, ct, depth), lc.to_8bit(lc.pixels(case), w, h, ct, depth, wrong="low-byte"))


@pytest.mark.parametrize("case", [c for c in lc.CASES if c[0] not in lc.SWEEP_CASES], ids=[n for n in lc.IDS if n not in lc.SWEEP_CASES])
def test_rules(exe, tmp_path, case):
    src_mod, dst_mod = _mods(case[0])
    _check(_run(exe, tmp_path, case, src_mod, dst_mod), case, "out of place")
    _check(_run(exe, tmp_path, case, dst_mod, src_mod ^ 1), case, "the other order")
    _check(_run(exe, tmp_path, case, src_mod, dst_mod, inplace=True), case, "in place")


def test_rules_beyond_a_sweep(exe, tmp_path):
    case = lc.case("run-sweep")
    _check(_run(exe, tmp_path, case, 4, 9), case, "out of place, falling")
    _check(_run(exe, tmp_path, case, 0, 0, inplace=True), case, "in place")


@pytest.mark.parametrize("name", ["run-tiles", "first-at-tile-m1", "ga-carry", "w7-ga", "w1-column", "rgba16-hi", "ga16-hi", "many-transparent-rgbs"])
def test_every_offset(exe, tmp_path, name):
    """Every address of the output mod 16, the image moving the other way; the workgroups in both orders; in place at
    every address."""
    case = lc.case(name)
    for dst_mod in range(16):
        _check(_run(exe, tmp_path, case, (7 * dst_mod + 3) % 16, dst_mod), case, dst_mod)
        _check(_run(exe, tmp_path, case, dst_mod, dst_mod, inplace=True), case, ("in place", dst_mod))


def test_sanitized_program(tmp_path):
    """The same program under AddressSanitizer and UBSan (host code, its own main): the image lies in a heap block that
    ends with its last byte, so a read beyond it is reported.  Every case, run-sweep's 25 MB included."""
    _make("SANITIZE=-fsanitize=address,undefined", "SUFFIX=_san")
    san = os.path.join(BUILD, "png_lossy_print_san")
    for case in lc.CASES:
        src_mod, dst_mod = _mods(case[0] + "san")
        _check(_run(san, tmp_path, case, src_mod, dst_mod), case, "sanitized")
        _check(_run(san, tmp_path, case, dst_mod, src_mod, inplace=True), case, "sanitized, in place")


# ---- against the all-reference zopflipng
def _reference(tmp_path, case, *flags):
    name, w, h, ct, depth = case
    src, dst = str(tmp_path / "in.png"), str(tmp_path / "ref.png")
    img = lc.pixels(case)
    bw = ec.CHANNELS[ct] * depth // 8
    with open(src, "wb") as f:
        f.write(ec.plain_png((w, h, ct, depth), filter_rows(img, bw, np.zeros(h, dtype=np.uint8))))
    r = subprocess.run([PNG_REF, "-y", "--always_zopflify", f"--iterations={ITERATIONS}", "--filters=0", *flags, src, dst],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-1000:])
    with open(dst, "rb") as f:
        return f.read()


def _need_reference():
    if not os.path.exists(PNG_REF) or not ol.have_ref():
        pytest.skip("oracle/_ref/zopflipng_ref not built (needs the reference's sources at build time)")


def _inflated(png):
    return zlib.decompress(dict(ec.chunks(png))[b"IDAT"])


@pytest.mark.parametrize("case", lc.CASES, ids=lc.IDS)
def test_model_is_zopflipngs(tmp_path, case):
    """Every case, the two large ones included: run-scan-step (3 MB) takes zopflipng about 2 s, run-sweep (25 MB) about
    13 s at 2 iterations; nothing smaller crosses the sweep of a full launch."""
    _need_reference()
    name, w, h, ct, depth = case
    bw = ec.CHANNELS[ct] * depth // 8
    ref = _reference(tmp_path, case, "--lossy_transparent", "--keepcolortype")
    # (rule 6: a 16-bit image is left alone)
    want = lc.pixels(case) if depth == 16 else lc.model(case)[1]
    assert _inflated(ref) == filter_rows(want, bw, np.zeros(h, dtype=np.uint8)).tobytes(), name
    assert ec.chunks(ref)[0][1][8:10] == bytes([depth, ct])


def _model_file(case, flags):
    """The file of the optimize entry under strategy 0, put together from png_color_cases' model on the prepared pixels and
    deflated by the reference's library: (file, whether the second try replaced the first: None where none is made)."""
    name, w, h, ct, depth = case
    img, d = lc.prepared(case, flags, True)
    rgba, st, mode = lc.reduced(img, w, h, ct, d)

    def file_in(m):
        scan = filter_rows(cc.convert(rgba, d, w, h, m), cc.bytewidth(m), np.zeros(h, dtype=np.uint8))
        return cc.assemble(w, h, m, ol.ref_compress(scan.tobytes(), 1, ITERATIONS))
    first = file_in(mode)
    if mode["colortype"] != 3 or len(first) >= cc.RETRY_BELOW:
        return first, None
    second = file_in(cc.retry_mode(st, w * h))
    return (second, True) if len(second) < len(first) else (first, False)


REF_FLAGS = {0: [], 1: ["--lossy_transparent"], 2: ["--lossy_8bit"], 3: ["--lossy_transparent", "--lossy_8bit"]}


@pytest.mark.parametrize("name", lc.ENTRY_CASES)
def test_entries_files_are_zopflipngs(tmp_path, name):
    _need_reference()
    case = lc.case(name)
    depth = case[4]
    for flags in ((0, 1, 2, 3) if depth == 16 else (0, 1)):
        ref = _reference(tmp_path, case, *REF_FLAGS[flags])
        want, retried = _model_file(case, flags)
        assert ref == want, (name, flags)
        if flags == 1 and name in lc.RETRY_EXPECT:
            assert retried == lc.RETRY_EXPECT[name], name
        # --keepcolortype: --lossy_8bit does nothing, --lossy_transparent nothing to a 16-bit image
        kept = _reference(tmp_path, case, "--keepcolortype", *REF_FLAGS[flags])
        img = lc.prepared(case, flags, False)[0]
        assert _inflated(kept) == filter_rows(img, ec.CHANNELS[case[3]] * depth // 8, np.zeros(case[2], dtype=np.uint8)).tobytes(), (name, flags)
