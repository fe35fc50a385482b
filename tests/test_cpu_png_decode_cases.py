"""The rules of device/zmx_png_decode.h on the CPU, through tests/hostlib/png_decode_print.cc, which runs the kernels' own
walks — the chunk walk, the skewed unfilter with its shift and band carry, the fused stores — with the 64 lanes one after
the other, built plain and with sanitizers.  png_decode_cases.py's reference decoder is held against LodePNG's recorded
verdicts and pixel hashes (tests/golden/png_decode.json) and against PIL where PIL decodes a mode exactly; then the program
against the reference on every case, field for field and byte for byte.  Every planted case must reach what its name says."""
import functools
import hashlib
import io
import json
import os
import subprocess
import zlib

import pytest

import png_decode_cases as pc
from zopfli_amd._build import ROOT

HOSTLIB_DIR = os.path.join(ROOT, "tests", "hostlib")
BUILD = os.path.join(ROOT, "tests", "_build")
GOLDEN = os.path.join(ROOT, "tests", "golden", "png_decode.json")
SHIFTS = [(0, 0), (1, 1), (3, 7), (15, 15)]
STREAM_DETAILS = {"stream_no_idat": 13, "stream_idat_empty": 13, "stream_bad_zlib_header": 1, "stream_block_type_3": 3, "stream_truncated": 13,
                  "stream_adler": 15}
FIELDS = ["status", "detail", "width", "height", "colortype", "bitdepth", "interlace", "palettesize", "has_key", "key_r", "key_g", "key_b",
          "outsize", "outsize_own", "outsize_rgba8"]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request):
    if request.param == "plain":
        subprocess.check_call(["make", "-s", "-C", HOSTLIB_DIR, "-f", "png_decode.mk"])
        return os.path.join(BUILD, "png_decode_print")
    subprocess.check_call(["make", "-s", "-C", HOSTLIB_DIR, "-f", "png_decode.mk", "SANITIZE=-fsanitize=address,undefined", "SUFFIX=_san"])
    return os.path.join(BUILD, "png_decode_print_san")


@functools.lru_cache(maxsize=None)
def reference(file, mode, capacity=None, size_only=False):
    return pc.decode_ref(file, mode, capacity, size_only)


def run(exe, jobs):
    """jobs: (mode, file, capacity or None, in_shift, out_shift, force_wide, entry_cap) -> the program's lines as lists of fields"""
    text = "".join(f"{mode} {'null' if cap is None else cap} {si} {so} {wide} {ecap} {file.hex() or '-'}\n" for mode, file, cap, si, so, wide, ecap in jobs)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    lines = [line.split() for line in r.stdout.splitlines()]
    assert len(lines) == len(jobs)
    return lines


def check_line(name, fields, ref, cap):
    """the program's line against the reference; what it wrote inside the destination"""
    got = dict(zip(FIELDS, (int(v) for v in fields[:15])))
    want = {k: ref[k] for k in FIELDS}
    if want["detail"] == -1:          # (a stream error the reference does not classify: the named cases settle it)
        want["detail"] = got["detail"]
    assert got == want, (name, pc.STATUS_NAMES[got["status"]])
    assert int(fields[15]) == zlib.crc32(ref["palette"]) & 0xffffffff, name
    write_lo, write_hi = fields[17:19]
    if ref["pixels"] is not None:
        assert int(fields[16]) == zlib.crc32(ref["pixels"]) & 0xffffffff, name
        assert (int(write_lo), int(write_hi)) == (0, len(ref["pixels"])), name
    elif write_lo != "-":
        # (an image that ends FILTER may have written the bands before the row, inside the destination)
        assert ref["status"] == pc.FILTER and cap is not None and 0 <= int(write_lo) and int(write_hi) <= min(cap, ref["outsize"]), name
        assert int(write_hi) <= (ref["detail"] // pc.LANES) * pc.LANES * (ref["outsize"] // ref["height"]), name


def test_constants_are_the_headers(exe):
    r = subprocess.run([exe, "constants"], capture_output=True, text=True)
    carry, entries, scratch, result_bytes = (int(v) for v in r.stdout.split())
    assert (carry, entries) == (pc.CARRY_BYTES, pc.ENTRIES)
    assert scratch == carry + 1024 and scratch <= 18 * 1024      # the carry row and the palette: eight waves a CU
    assert result_bytes == 12 * 4 + 3 * 8 + 1024


def test_reference_equals_lodepng_golden():
    """LodePNG's own verdicts and pixels, recorded by tests/golden/make_png_decode_golden.py: the hashes of both modes on every
    valid case, a nonzero error exactly where the reference refuses"""
    with open(GOLDEN) as f:
        golden = json.load(f)
    cases = pc.valid_cases()
    assert sorted(golden["valid"]) == sorted(c.name for c in cases)
    for case in cases:
        g = golden["valid"][case.name]
        assert g["file_sha256"] == hashlib.sha256(case.file).hexdigest(), case.name      # (the writer is byte-stable)
        if case.name in pc.LODEPNG_REFUSES:
            assert g["error"] == pc.LODEPNG_REFUSES[case.name] and reference(case.file, pc.OWN)["status"] == pc.OK
            continue
        for mode, key in ((pc.OWN, "own"), (pc.RGBA8, "rgba8")):
            ref = reference(case.file, mode)
            assert ref["status"] == pc.OK, case.name
            assert hashlib.sha256(ref["pixels"]).hexdigest() == g[key], (case.name, key)
    bad = pc.malformed_cases() + pc.truncation_cases()
    assert sorted(golden["malformed"]) == sorted(b.name for b in bad)
    for b in bad:
        g = golden["malformed"][b.name]
        assert bytes.fromhex(g["file"]) == b.file, b.name
        ref = reference(b.file, pc.OWN)
        if b.name == "interlaced_valid":
            assert g["error"] == 0 and ref["status"] == pc.INTERLACE       # (the stated exception: recognised, not decoded)
            continue
        assert g["error"] != 0 and ref["status"] != pc.OK, (b.name, g["error"], ref["status"])


def test_reference_equals_pil():
    from PIL import Image
    exact_own = {(0, 8), (2, 8), (4, 8), (6, 8), (3, 8)}
    seen = 0
    for case in pc.valid_cases():
        if case.name in ("idat_not_adjacent", "ancillary_wrong_crcs", "ancillary_unknown_wrong_crcs"):
            continue        # (PIL wants IDATs adjacent and every CRC right; LodePNG and this library do not)
        own, rgba = reference(case.file, pc.OWN), reference(case.file, pc.RGBA8)
        im = Image.open(io.BytesIO(case.file))
        im.load()
        pair = (own["colortype"], own["bitdepth"])
        if pair in exact_own:
            assert im.tobytes() == own["pixels"], case.name
            seen += 1
        if pair == (6, 8):
            assert im.tobytes() == rgba["pixels"], case.name
        if pair[0] == 3 and case.name != "palette_index_above_size":
            assert im.convert("RGBA").tobytes() == rgba["pixels"], case.name
    assert seen >= 60


def test_cases_reach_what_their_names_say():
    paeth, avg9, row0, seam, first = set(), set(), {}, {}, set()
    pairs = set()
    for case in pc.valid_cases():
        ref = reference(case.file, pc.OWN)
        assert ref["status"] == pc.OK, case.name
        t = ref["trace"]
        pair = (ref["colortype"], ref["bitdepth"])
        pairs.add(pair)
        paeth |= t["paeth"]
        avg9 |= t["avg9"]
        first |= {(pc.bytewidth_of(*pair), k) for k in t["first"]}
        row0.setdefault(pair, set()).update(t["row0"])
        seam.setdefault(pair, set()).update(t["seam"])
    assert pairs == set(pc.LEGAL)
    widths = {1, 2, 3, 4, 6, 8}
    for bw in widths:
        # every choice of Paeth's, and every tie: a and b, b and c, a and c, all three
        assert {(w, tie) for b, w, tie in paeth if b == bw} >= {("a", "none"), ("b", "none"), ("c", "none"), ("a", "ab"), ("b", "bc"), ("a", "ac"),
                                                                ("a", "all")}, bw
        assert bw in avg9
        assert {(bw, 1), (bw, 3)} <= first
    for pair in pc.LEGAL:
        assert row0[pair] == {0, 1, 2, 3, 4} and seam[pair] == {0, 1, 2, 3, 4}, pair      # every type on row 0 and on a band's first row
    geometry = {(reference(c.file, pc.OWN)["width"], reference(c.file, pc.OWN)["height"]) for c in pc.filter_cases()}
    assert {w for w, _ in geometry} == set(pc.WIDTHS) and {h for _, h in geometry} == set(pc.HEIGHTS)
    by_name = {c.name: c for c in pc.valid_cases()}
    assert reference(by_name["idat_more_than_capacity"].file, pc.OWN)["nentries"] > pc.ENTRIES
    assert {b.status for b in pc.malformed_cases()} == set(range(1, 12))      # one file at least per line of the status table (CAPACITY: below)
    for b in pc.malformed_cases():
        ref = reference(b.file, pc.OWN)
        assert ref["status"] == b.status, (b.name, pc.STATUS_NAMES[ref["status"]])
        if b.name in pc.FILTER_ROWS:
            assert ref["detail"] == pc.FILTER_ROWS[b.name]
    # the 16-bit key cases hold a pixel equal to the key in its high bytes only: opaque, beside one that is transparent
    for name in ("key_grey_16", "key_rgb_16"):
        px = reference(by_name[name].file, pc.RGBA8)["pixels"]
        alphas = px[3::4]
        assert 0 in alphas
        rgb = [px[i:i + 3] for i in range(0, len(px), 4)]
        clear = {rgb[i] for i, a in enumerate(alphas) if a == 0}
        assert any(a == 255 and rgb[i] in clear for i, a in enumerate(alphas)), name


def test_programs_equal_the_reference_on_valid_files(exe):
    cases = pc.valid_cases()
    for mode in (pc.OWN, pc.RGBA8):
        jobs = [(mode, c.file, reference(c.file, mode)["outsize"], *SHIFTS[i % 4], c.hooks["force_wide"], c.hooks["entry_cap"])
                for i, c in enumerate(cases)]
        for case, fields in zip(cases, run(exe, jobs)):
            check_line(case.name, fields, reference(case.file, mode), None)
            assert int(fields[20]) == case.hooks["force_wide"], case.name
            walks = 2 if reference(case.file, mode)["nentries"] > (case.hooks["entry_cap"] or pc.ENTRIES) else 1
            assert int(fields[19]) == walks, case.name


def test_every_file_takes_the_wide_path_too(exe):
    """the band carry through global rows gives the same bytes as the LDS row"""
    cases = [c for c in pc.valid_cases() if reference(c.file, pc.OWN)["height"] > pc.LANES]
    jobs = [(i % 2, c.file, reference(c.file, i % 2)["outsize"], *SHIFTS[(i + 1) % 4], 1, 0) for i, c in enumerate(cases)]
    for i, (case, fields) in enumerate(zip(cases, run(exe, jobs))):
        check_line(case.name, fields, reference(case.file, i % 2), None)
        assert int(fields[20]) == 1


def test_programs_equal_the_reference_on_malformed_files(exe):
    cases = pc.malformed_cases() + pc.truncation_cases()
    jobs = [(i % 2, b.file, 4096, i % 16, (5 * i) % 16, 0, 0) for i, b in enumerate(cases)]
    for i, (b, fields) in enumerate(zip(cases, run(exe, jobs))):
        ref = reference(b.file, i % 2, 4096)
        assert ref["status"] != pc.OK, b.name
        check_line(b.name, fields, ref, 4096)
        if b.name in STREAM_DETAILS:
            assert int(fields[1]) == STREAM_DETAILS[b.name], b.name


def test_size_only_and_short_capacities(exe):
    """The size-only mode writes nothing and fills the same fields; a capacity below the size — one byte short, none — gives
    CAPACITY with the size and writes nothing."""
    cases = pc.planted_cases()
    jobs, what = [], []
    for i, case in enumerate(cases):
        mode = i % 2
        n = reference(case.file, mode)["outsize"]
        for cap in (None, n - 1, 0):
            jobs.append((mode, case.file, cap, i % 16, (3 * i) % 16, case.hooks["force_wide"], case.hooks["entry_cap"]))
            what.append((case, mode, cap))
    for (case, mode, cap), fields in zip(what, run(exe, jobs)):
        ref = reference(case.file, mode, cap, cap is None)
        check_line(case.name, fields, ref, cap)
        assert int(fields[0]) == (pc.OK if cap is None else pc.CAPACITY), case.name
        assert fields[17] == "-", case.name
    # a wrong Adler-32 shows only where the scanlines are stored
    adler = next(b for b in pc.malformed_cases() if b.name == "stream_adler")
    fields = run(exe, [(0, adler.file, None, 0, 0, 0, 0)])[0]
    assert int(fields[0]) == pc.OK
