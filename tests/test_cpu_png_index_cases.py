"""Palette, 1/2/4-bit grey and index images on the CPU.  The rules of zopfli_amd/csrc/device/zmx_png_index.h and
zopfli_amd/csrc/host/png_index.h are run by tests/hostlib/png_index_print.cc, the threads of a launch one after the other,
on every case of tests/png_index_cases.py: the first-appearance table, the derived statistics, the mode, the table and the
converted bytes must be the numpy model's — the statistics also png_color_cases.stats of the RGBA8 expansion, the
converted bytes also png_color_cases.convert of it — at every alignment, the workgroups in both orders, with the guard
bytes around the output and the image left as they were.  The same program runs under AddressSanitizer and UBSan.  The
model's --keepcolortype files are held against the all-reference zopflipng where it was built, and always against
tests/golden/png_index.json."""
import json
import os
import subprocess
import zlib

import numpy as np
import pytest

import oracle_lib as ol
import png_color_cases as cc
import png_encode_cases as ec
import png_index_cases as ic
from png_rows_cases import filter_rows
from zopfli_amd._build import PNG_REF, ROOT

HOSTLIB_DIR = os.path.join(ROOT, "tests", "hostlib")
BUILD = os.path.join(ROOT, "tests", "_build")
GOLDEN = os.path.join(ROOT, "tests", "golden", "png_index.json")
WHATS = ("keep", "optimize", "retry")


def _make(*extra):
    subprocess.check_call(["make", "-s", "-C", HOSTLIB_DIR, "-f", "png_index.mk", *extra])


@pytest.fixture(scope="module")
def exe():
    _make()
    return os.path.join(BUILD, "png_index_print")


def _hex_palette(case):
    return "-" if case[3] != 3 else ic.palette_of(case).tobytes().hex()


def _run(exe, tmp_path, case, src_mod, dst_mod, lossy, what):
    """png_index_print on a case: the lines it printed by their first word, and the converted rows."""
    name, w, h, ct, depth, _ = case
    src, out = os.path.join(str(tmp_path), "in.bin"), os.path.join(str(tmp_path), "out.bin")
    with open(src, "wb") as f:
        f.write(ic.packed(case).tobytes())
    r = subprocess.run([exe, src, out, str(src_mod), str(dst_mod), str(w), str(h), str(ct), str(depth), _hex_palette(case), str(lossy), what],
                       capture_output=True, text=True)
    assert r.returncode == 0, (name, r.stdout[-2000:], r.stderr[-2000:])
    lines = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines()}
    assert "ok" in lines, r.stdout
    return lines, np.fromfile(out, dtype=np.uint8).reshape(h, -1)


def _mods(name):
    k = zlib.crc32(name.encode())
    return (k >> 4) % 16, (k >> 8) % 16


def _palette(hexed):
    return np.zeros((0, 4), dtype=np.uint8) if hexed == "-" else np.frombuffer(bytes.fromhex(hexed), dtype=np.uint8).reshape(-1, 4)


def _want_mode(case, lossy, what):
    _, w, h, _, _, _ = case
    st = cc.stats(ic.expand(case, lossy), 8)
    if what == "keep":
        return st, ic.keep_mode(case, lossy)
    return st, (cc.choose(st, w * h) if what == "optimize" else cc.retry_mode(st, w * h))


def _check(got, case, lossy, what):
    lines, rows = got
    name, w, h, ct, depth, _ = case
    first = [ic.UNUSED if int(x) < 0 else int(x) for x in lines["first"]]
    assert first == ic.first_table(ic.values(case)), (name, "first appearances")
    assert lines["outside"] == ["-1"] and lines["bad"] == ["-1"]
    st, mode = _want_mode(case, lossy, what)
    s = lines["stats"]
    assert [int(x) for x in s[:5]] == [int(st["colored"]), int(st["key"]), int(st["alpha"]), st["numcolors"], st["bits"]], (name, lossy, s)
    assert tuple(int(x) for x in s[5:8]) == st["key_rgb"]
    assert np.array_equal(_palette(s[8]), st["palette"]), (name, "the colours in first-appearance order")
    m = lines["mode"]
    key = tuple(int(x) for x in m[4:7]) if int(m[3]) else None
    assert (int(m[0]), int(m[1]), key) == (mode["colortype"], mode["bitdepth"], mode["key"]), (name, lossy, what, m)
    if mode["colortype"] == 3:
        assert np.array_equal(_palette(m[7]), np.asarray(mode["palette"])), (name, lossy, what)
    table = [int(x) for x in lines["table"]]
    n = len(ic.palette_of(case))
    want_table = ic.table_for(ic.seen_palette(case, lossy), mode)
    used = [v for v in range(n) if first[v] != ic.UNUSED]
    assert [table[v] for v in used] == [want_table[v] for v in used], (name, lossy, what)
    assert np.array_equal(rows, ic.convert_table(ic.values(case), want_table, mode)), (name, lossy, what, "the table-driven conversion")
    assert np.array_equal(rows, cc.convert(ic.expand(case, lossy), 8, w, h, mode)), (name, lossy, what, "LodePNG's conversion of the expansion")
    assert 1 <= int(lines["ok"][0]) <= 2048 and 1 <= int(lines["ok"][1]) <= 2048


@pytest.mark.parametrize("case", ic.CASES, ids=ic.IDS)
def test_model_reaches_what_the_case_is_for(case):
    name, w, h, ct, depth, _ = case
    vals = ic.values(case)
    assert vals.shape == (h, w) and int(vals.max()) < len(ic.palette_of(case))
    per = 8 // depth
    if w % per:
        # (garbage in the padding bits: a kernel that counted them, or copied them, would be seen)
        assert np.all(ic.packed(case)[:, -1] & ((1 << ((per - w % per) * depth)) - 1))
    got = tuple(ic.mode_tuple(_want_mode(case, lossy, "optimize")[1]) for lossy in (0, 1))
    if name in ic.EXPECT:
        assert got == (ic.EXPECT[name], ic.LOSSY_EXPECT.get(name, ic.EXPECT[name])), (name, got)
    if name in ic.KEEP_PALETTE:
        assert tuple(len(ic.keep_mode(case, lossy)["palette"]) for lossy in (0, 1)) == ic.KEEP_PALETTE[name], name
    first = ic.first_table(vals)
    if name == "last-pixel":
        assert first[2] == w * h - 1
    if name == "big8":
        assert all(f != ic.UNUSED for f in first) and max(first) < 256
        # (4096 bytes a workgroup: every value lies in several workgroups' shares)
        assert all(np.count_nonzero(vals.reshape(-1)[4096:] == v) > 1 for v in range(256))
    if name == "two-equal":
        assert first[2] < first[0] != ic.UNUSED
        st = cc.stats(ic.expand(case), 8)
        assert st["numcolors"] == 3 and tuple(st["palette"][1]) == ic.FOUR[0]   # born at min(first[0], first[2]) = pixel 1
        assert ic.table_for(ic.palette_of(case), ic.keep_mode(case))[0] == 2    # the keep path maps to the later index
    if name == "two-transparent":
        assert len(np.unique(ic.expand(case, 0), axis=0)) == 5 and len(np.unique(ic.expand(case, 1), axis=0)) == 4
        assert first[3] < first[1]   # (the second transparent entry comes first: its RGB is the one kept)
        assert [tuple(e) for e in ic.keep_mode(case, 1)["palette"]] == [ic.FOUR[0], ic.FOUR[1], (40, 50, 60, 0), ic.FOUR[2]]
    if name == "unused":
        assert sum(f != ic.UNUSED for f in first) == 3


@pytest.mark.parametrize("case", ic.CASES, ids=ic.IDS)
def test_rules(exe, tmp_path, case):
    src_mod, dst_mod = _mods(case[0])
    for lossy in (0, 1):
        for k, what in enumerate(WHATS):
            _check(_run(exe, tmp_path, case, (src_mod + k) % 16, (dst_mod + 5 * k + lossy) % 16, lossy, what), case, lossy, what)


@pytest.mark.parametrize("name", ["b1-w17-h3", "b2-w5-h3", "b4-w3-h3", "two-equal", "grey-key"])
def test_every_offset(exe, tmp_path, name):
    """Every address of the output mod 16, the image moving the other way; the workgroups in both orders."""
    case = ic.case(name)
    for dst_mod in range(16):
        _check(_run(exe, tmp_path, case, (7 * dst_mod + 3) % 16, dst_mod, dst_mod & 1, WHATS[dst_mod % 3]), case, dst_mod & 1, WHATS[dst_mod % 3])


@pytest.mark.parametrize("case,at", ic.OUTSIDE, ids=[c[0][0] for c in ic.OUTSIDE])
def test_value_outside_the_palette(exe, tmp_path, case, at):
    """The first-appearance table shows it to the host, and the convert kernel reports the same pixel."""
    lines, _ = _run(exe, tmp_path, case, 3, 6, 0, "keep")
    assert lines["outside"] == [str(at)] and lines["bad"] == [str(at)]
    assert "stats" not in lines


def test_sanitized_program(tmp_path):
    """The same program under AddressSanitizer and UBSan (host code, its own main): the image lies in a heap block that
    ends with its last byte, so a read beyond it is reported."""
    _make("SANITIZE=-fsanitize=address,undefined", "SUFFIX=_san")
    san = os.path.join(BUILD, "png_index_print_san")
    for case in ic.CASES:
        src_mod, dst_mod = _mods(case[0] + "san")
        for lossy, what in ((0, "keep"), (1, "optimize"), (1, "keep"), (0, "retry")):
            _check(_run(san, tmp_path, case, src_mod, dst_mod ^ lossy, lossy, what), case, lossy, what)
    for case, at in ic.OUTSIDE:
        assert _run(san, tmp_path, case, 1, 2, 0, "keep")[0]["bad"] == [str(at)]


# ---- against the all-reference zopflipng
def _keep_file_parts(png):
    """(IHDR's depth and colour type, PLTE, tRNS, the inflated IDAT) of a file."""
    ch = dict(ec.chunks(png))
    return ch[b"IHDR"][8:10], ch.get(b"PLTE"), ch.get(b"tRNS"), zlib.decompress(ch[b"IDAT"])


def _model_keep_parts(case, lossy):
    name, w, h, ct, depth, _ = case
    mode = ic.keep_mode(case, lossy)
    rows = ic.convert_table(ic.values(case), ic.table_for(ic.seen_palette(case, lossy), mode), mode)
    plte = trns = None
    if ct == 3:
        pal = np.asarray(mode["palette"])
        plte = pal[:, :3].tobytes()
        notopaque = np.nonzero(pal[:, 3] != 255)[0]
        trns = pal[: notopaque[-1] + 1, 3].tobytes() if len(notopaque) else None
    return bytes([depth, ct]), plte, trns, filter_rows(rows, 1, np.zeros(h, dtype=np.uint8)).tobytes()


@pytest.mark.parametrize("case", ic.SMALL, ids=[c[0] for c in ic.SMALL])
def test_keep_model_is_zopflipngs(case):
    """--keepcolortype --filters=0 [--lossy_transparent]: the mode, the palette in the input's order (shrunk after the lossy
    rewrite), tRNS and the rows — duplicates mapped to the later index, padding bits zero — from the recorded files."""
    with open(GOLDEN) as f:
        golden = json.load(f)
    for lossy in (0, 1):
        ref = bytes.fromhex(golden["files"][f"{case[0]}|keep|0|{lossy}"])
        assert _keep_file_parts(ref) == _model_keep_parts(case, lossy), (case[0], lossy)


@pytest.mark.parametrize("case", ic.SMALL, ids=[c[0] for c in ic.SMALL])
def test_golden_is_the_reference(tmp_path, case):
    if not os.path.exists(PNG_REF) or not ol.have_ref():
        pytest.skip("oracle/_ref/zopflipng_ref not built (needs the reference's sources at build time)")
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_png_index_golden as mk
    with open(GOLDEN) as f:
        golden = json.load(f)
    for keep in (True, False):
        for lossy in (0, 1):
            key = f"{case[0]}|{'keep' if keep else 'optimize'}|0|{lossy}"
            assert mk.reference(str(tmp_path), case, "0", keep, lossy).hex() == golden["files"][key], key
