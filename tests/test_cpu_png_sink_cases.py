"""Decoding into strided, planar, float and 16-bit sinks on the CPU.  The numpy model of tests/png_sink_cases.py is held
against what the real lodepng_convert gave (tests/golden/png_sink.json) on every file and each of the 8 output modes, and
must tell six wrong models from the right one; the rules of zopfli_amd/csrc/device/zmx_png_unpack.h and
zopfli_amd/csrc/host/png_sink.h are run by tests/hostlib/png_sink_print.cc, the threads of a launch one after the other and
in both orders, on every case — singly and as one batch —: every allocation must be the model's byte for byte, guard and
gap bytes as they were, every byte of every sample written exactly once and no other.  The same program runs under
AddressSanitizer and UBSan.  The host checks: every refusal that needs no device, with the index in the message."""
import hashlib
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import png_sink_cases as sk
from zopfli_amd._build import ROOT

HOSTLIB_DIR = os.path.join(ROOT, "tests", "hostlib")
BUILD = os.path.join(ROOT, "tests", "_build")
GOLDEN = os.path.join(ROOT, "tests", "golden", "png_sink.json")


def _make(*extra):
    subprocess.check_call(["make", "-s", "-C", HOSTLIB_DIR, "-f", "png_sink.mk", *extra])


@pytest.fixture(scope="module")
def exe():
    _make()
    return os.path.join(BUILD, "png_sink_print")


@pytest.fixture(scope="module")
def tile(exe):
    """a tile's pixels, as the header's own program prints them"""
    return int(subprocess.check_output([exe, "constants"], text=True).split()[0])


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def record(file, sink, fake=0, base_mod=0, own_mod=0):
    """a case as tests/hostlib/png_sink_print.cc reads it"""
    if file is None:
        m, own = dict(width=sink.width, height=sink.height, colortype=0, bitdepth=8, palettesize=0, has_key=0, key_r=0, key_g=0, key_b=0, palette=bytes(1024)), b""
    else:
        m, own = sk.mode_of(file)
    head = struct.pack("<9I", m["width"], m["height"], m["colortype"], m["bitdepth"], m["palettesize"], m["has_key"], m["key_r"], m["key_g"], m["key_b"])
    return head + m["palette"] + sink.record(fake, base_mod) + struct.pack("<IQ", own_mod, len(own)) + own


def run(exe, tmp_path, records, falling=0):
    src, out = os.path.join(str(tmp_path), "in.bin"), os.path.join(str(tmp_path), "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<I", len(records)))
        for r in records:
            f.write(r)
    r = subprocess.run([exe, src, out, str(falling)], capture_output=True, text=True)
    data = open(out, "rb").read() if os.path.exists(out) else b""
    return r.returncode, r.stdout.splitlines(), data


def check_stored(exe, tmp_path, cases, falling, salt=0):
    """the cases singly and as one batch: the model's bytes, and every sample byte written exactly once, no other"""
    records = [record(c.file, c.sink, base_mod=4 * ((k + salt) % 4), own_mod=(5 * k + salt) % 16) for k, c in enumerate(cases)]
    rc, lines, data = run(exe, tmp_path, records, falling)
    assert rc == 0 and lines[-1] == "ok", lines[-5:]
    at = 0
    for what in ("single", "batch"):
        for c in cases:
            n = c.sink.buflen
            got, counts = np.frombuffer(data, np.uint8, n, at), np.frombuffer(data, np.uint8, n, at + n)
            at += 2 * n
            want = c.sink.expected(*sk.mode_of(c.file))
            assert np.array_equal(counts, c.sink.written()), (c.name, what, "write counts differ at", int(np.flatnonzero(counts != c.sink.written())[0]))
            assert np.array_equal(got, want), (c.name, what, "first difference at", int(np.flatnonzero(got != want)[0]))
    assert at == len(data)
    return lines


# ---- the model against LodePNG
def test_model_is_lodepng_convert(golden):
    """every file, each of the 8 output modes: the SHA-256 of the model's image is that of lodepng_convert's"""
    files = sk.all_files()
    assert sorted(golden) == sorted(f.name for f in files)
    for f in files:
        g = golden[f.name]
        assert hashlib.sha256(f.file).hexdigest() == g["file_sha256"], f.name
        m, own = sk.mode_of(f.file)
        for channels, depth in sk.MODES:
            got = hashlib.sha256(sk.lodepng_bytes(sk.values(m, own, channels, depth), depth)).hexdigest()
            assert got == g[f"c{channels}_d{depth}"], (f.name, channels, depth)


@pytest.mark.parametrize("wrong", sk.WRONG)
def test_cases_tell_a_wrong_model(tile, wrong):
    differing = 0
    for c in sk.cases(tile):
        m, own = sk.mode_of(c.file)
        differing += not np.array_equal(c.sink.expected(m, own, wrong), c.sink.expected(m, own))
    assert differing, wrong


def test_files_hold_what_the_conversion_turns_on():
    """all 15 pairs; keys met at full depth and in the high byte alone; a palette index at or above palettesize; every
    low-bit grey value; 16-bit samples whose bytes differ"""
    modes = [sk.mode_of(f.file) for f in sk.extra_files()]
    assert {(m["colortype"], m["bitdepth"]) for m, _ in modes} == set(sk.pc.LEGAL)
    for f in sk.extra_files():
        m, own = sk.mode_of(f.file)
        s = sk.file_samples(m, own)
        if f.name.startswith("key_") and m["bitdepth"] == 16:
            keys = np.array([m["key_r"], m["key_g"], m["key_b"]], dtype=np.uint32)[:s.shape[2]]
            full, high = (s == keys).all(axis=2), ((s >> 8) == (keys >> 8)).all(axis=2)
            assert full.any() and (high & ~full).any(), f.name
        if f.name.startswith("palette"):
            assert (s >= m["palettesize"]).any() and (s < m["palettesize"]).any(), f.name
        if f.name.startswith("grey_") and f.name.endswith("every_value"):
            assert set(s.reshape(-1).tolist()) == set(range(1 << m["bitdepth"])), f.name
        if f.name.startswith("low_bytes"):
            assert ((s >> 8) != (s & 255)).all(), f.name


# ---- the kernel's rules, thread by thread
def _chunks(cases, n=4):
    return [cases[k::n] for k in range(n)]


@pytest.mark.parametrize("chunk", range(4))
@pytest.mark.parametrize("falling", (0, 1))
def test_rules(exe, tmp_path, tile, chunk, falling):
    check_stored(exe, tmp_path, _chunks(sk.cases(tile))[chunk], falling, salt=chunk + falling)


def test_cases_reach_every_path_type_and_seam(exe, tmp_path, tile):
    """all three paths with every sample type and depth and every channel count; one tile, two, a row across a tile's end"""
    cases = sk.cases(tile)
    lines = check_stored(exe, tmp_path, cases[::3], 0)
    runs = [ln.split() for ln in lines if ln.startswith("run ")]
    seen = {(cases[::3][int(i)].sink.sample, cases[::3][int(i)].sink.depth, int(path)) for _, i, path, _ in runs}
    assert seen == {(s, d, p) for s, d in sk.COMBOS for p in (0, 1, 2)}
    every = {(c.sink.channels, c.sink.sample, c.sink.depth) for c in cases}
    assert every == {(n, s, d) for n in (1, 2, 3, 4) for s, d in sk.COMBOS}
    shapes = {(c.sink.width, c.sink.height) for c in cases}
    assert {(tile - 1, 1), (tile + 1, 1), (tile // 2 + 24, 3)} <= shapes
    assert tile % (tile // 2 + 24) != 0                      # (the tile's end falls inside a row)
    assert {w for w, _ in shapes} >= {1, 3, 5, 15, 16, 17, 63, 64, 65} and {h for _, h in shapes} >= {1, 2, 65}


def test_nchw_batch_of_unlike_images(exe, tmp_path):
    """five images of one size into ONE (N, C, H, W) allocation: the program is given each sink with the shared allocation's
    size, so every image's stores are held to its own samples and the bytes of the others stay as they were"""
    files = [f for f in sk.extra_files() if f.name.startswith("pair_")][:5]
    for sample, depth in ((sk.F32, 8), (sk.U16, 16)):
        _, sinks = sk.batch_nchw(files, sample, depth)
        check_stored(exe, tmp_path, [sk.Case(f.name + ">" + s.name, f.file, s) for f, s in zip(files, sinks)], 0)


def test_sanitized_program(tmp_path, tile):
    """the same program under AddressSanitizer and UBSan (host code, its own main): every allocation and every image is a
    heap block that ends with its last byte"""
    _make("SANITIZE=-fsanitize=address,undefined", "SUFFIX=_san")
    check_stored(os.path.join(BUILD, "png_sink_print_san"), tmp_path, sk.cases(tile)[::2], 1, salt=3)


# ---- the host checks
def _checked(exe, tmp_path, sinks, fake=1 << 40):
    rc, lines, _ = run(exe, tmp_path, [record(None, s, fake=fake) for s in sinks])
    assert rc == 0, lines
    return [ln.split(None, 2) for ln in lines if ln.startswith("check ")]


def test_refusals_that_need_no_device(exe, tmp_path):
    refused = sk.refusals()
    got = _checked(exe, tmp_path, [s for s, _ in refused])
    assert len(got) == len(refused)
    for k, ((_, index, line), (_, text)) in enumerate(zip(got, refused)):
        assert int(index) == k and not line.startswith("ok") and text in line, (k, line, text)
    assert "null pointer" in _checked(exe, tmp_path, [sk.accepted()[0]], fake=1)[0][2]
    fine = _checked(exe, tmp_path, sk.accepted())
    assert all(line.startswith("ok") for _, _, line in fine), fine


def test_extent_is_the_samples_span(exe, tmp_path, tile):
    """[lo, hi) against the offsets the model scatters to, for every layout of the cases"""
    sinks = {c.sink.name: c.sink for c in sk.cases(tile)}.values()
    got = _checked(exe, tmp_path, list(sinks))
    for s, (_, _, line) in zip(sinks, got):
        at = s.sample_bytes()
        assert line == f"ok {at.min() - s.offset} {at.max() + 1 - s.offset}", (s.name, line)


# ---- the round trip of the values
def _source_quantise(x32, depth):
    """the source's rule (include/zopfli_amd.h): (uint32) clamp(fl32(fl32(x * maxv) + 0.5f), 0, maxv)"""
    maxv = np.float32(255.0 if depth == 8 else 65535.0)
    a = x32 * maxv + np.float32(0.5)
    assert a.dtype == np.float32
    return np.clip(a, 0, maxv).astype(np.int64)


# which (sample, depth) give every value back: found by enumeration below, asserted for those it holds for
ROUND_TRIP_HOLDS = {(sk.F32, 8): True, (sk.F32, 16): True, (sk.F16, 8): True, (sk.BF16, 8): True, (sk.F16, 16): False, (sk.BF16, 16): False}


@pytest.mark.parametrize("sample,depth", sorted(ROUND_TRIP_HOLDS))
def test_round_trip_of_every_value(sample, depth):
    """the sink's float of v, quantised by the source's rule, is v again — for every v of the depth, where the type can hold
    that many values; float16 and bfloat16 at 16 bits cannot, and the test says how many values survive"""
    v = np.arange(1 << depth, dtype=np.uint32)
    raw = sk.samples(v, sample, depth)
    if sample == sk.F32:
        x = raw.view("<f4").reshape(-1)
    elif sample == sk.F16:
        x = raw.view("<f2").reshape(-1).astype(np.float32)
    else:
        x = (raw.view("<u2").reshape(-1).astype(np.uint32) << 16).view(np.float32)
    back = _source_quantise(x, depth)
    holds = bool(np.array_equal(back, v))
    print(sk.SAMPLE_NAMES[sample], depth, "values that come back:", int((back == v).sum()), "of", len(v))
    assert holds == ROUND_TRIP_HOLDS[(sample, depth)]
