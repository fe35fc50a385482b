"""Strided, planar, float and 16-bit sources on the CPU.  The numpy model of tests/png_source_cases.py is held against torch's
CPU arithmetic and must tell ten wrong models from the right one; the rules of zopfli_amd/csrc/device/zmx_png_pack.h and
zopfli_amd/csrc/host/png_source.h are run by tests/hostlib/png_source_print.cc, the threads of a launch one after the other
and the workgroups in both orders, on every case — singly and as one batch whose destinations share 16-byte vectors —: the
packed bytes must be the model's, the guard bytes and the sources as they were.  The same program runs under
AddressSanitizer and UBSan.  The host checks: every refusal that needs no device, the extent for all eight sign
combinations of the strides, 64-bit overflow."""
import itertools
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import png_source_cases as sc
from zopfli_amd._build import ROOT

HOSTLIB_DIR = os.path.join(ROOT, "tests", "hostlib")
BUILD = os.path.join(ROOT, "tests", "_build")


def _make(*extra):
    subprocess.check_call(["make", "-s", "-C", HOSTLIB_DIR, "-f", "png_source.mk", *extra])


@pytest.fixture(scope="module")
def exe():
    _make()
    return os.path.join(BUILD, "png_source_print")


@pytest.fixture(scope="module")
def want():
    """The model's bytes of every case, made once."""
    return {c.name: sc.pack(c) for c in sc.CASES}


def _mods(name, salt=0):
    k = zlib.crc32(name.encode()) + 97 * salt
    return 4 * ((k >> 4) % 4), (k >> 8) % 16


def _run(exe, tmp_path, records, falling=0):
    src, out = os.path.join(str(tmp_path), "in.bin"), os.path.join(str(tmp_path), "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<I", len(records)))
        for r in records:
            f.write(r)
    r = subprocess.run([exe, src, out, str(falling)], capture_output=True, text=True)
    lines = r.stdout.splitlines()
    data = open(out, "rb").read() if os.path.exists(out) else b""
    return r.returncode, lines, data


def _check_packed(exe, tmp_path, cases, want, salt, falling):
    """The cases singly and as one batch: both must give the model's bytes."""
    records = [c.record(*_mods(c.name, salt)) for c in cases]
    rc, lines, data = _run(exe, tmp_path, records, falling)
    assert rc == 0 and lines[-1] == "ok", lines[-5:]
    at = 0
    for what in ("single", "batch"):
        for c in cases:
            got = data[at:at + c.nbytes]
            assert got == want[c.name], (c.name, what, "first difference at", next(i for i in range(c.nbytes) if got[i:i + 1] != want[c.name][i:i + 1]))
            at += c.nbytes
    assert at == len(data)
    return lines


# ---- the model
def _torch_quantise(x32, depth):
    import torch
    maxv = 255.0 if depth == 8 else 65535.0
    t = torch.from_numpy(np.ascontiguousarray(x32)).clone()
    t = t.mul(maxv).add_(0.5).clamp_(0, maxv)
    return torch.nan_to_num(t, nan=0.0).to(torch.int64).numpy()


@pytest.mark.parametrize("case", [c for c in sc.CASES if c.sample in (sc.F16, sc.BF16, sc.F32)], ids=repr)
def test_model_is_torchs_arithmetic(case):
    """mul(maxv).add_(0.5).clamp_(0, maxv), a NaN 0, truncated: torch's CPU result on every float case."""
    raw = sc.gather(case)
    got = sc.quantise(raw, case.sample, case.depth)
    assert np.array_equal(got, _torch_quantise(sc.to_float32(np.ascontiguousarray(raw), case.sample), case.depth))


def test_f16_and_bf16_are_widened_exactly():
    import torch
    bits = np.arange(65536, dtype=np.uint16)
    for sample, dtype in ((sc.F16, torch.float16), (sc.BF16, torch.bfloat16)):
        want = torch.from_numpy(bits.view(np.int16)).view(dtype).to(torch.float32).numpy().view(np.uint32)
        got = sc.to_float32(bits.astype(np.uint32), sample).view(np.uint32)
        nan = np.isnan(got.view(np.float32))
        assert np.array_equal(got[~nan], want[~nan]) and np.all(np.isnan(want.view(np.float32))[nan])


@pytest.mark.parametrize("wrong", sc.WRONG)
def test_cases_tell_a_wrong_model(want, wrong):
    differing = [c.name for c in sc.CASES if sc.pack(c, wrong) != want[c.name]]
    assert differing, wrong


def test_double_arithmetic_differs_where_measured():
    """The rule is not exact arithmetic: the ties' neighbours hold inputs on which double differs, at both depths."""
    for depth in (8, 16):
        raw = sc.ties(depth)
        assert np.count_nonzero(sc.quantise(raw, sc.F32, depth) != sc.quantise(raw, sc.F32, depth, "double")) > 0


def test_cases_reach_every_path_and_edge(exe, tmp_path):
    """What the builders promise: all three paths with every sample type and depth, one, two and many tiles, one byte."""
    records = [c.record(0, 0) for c in sc.SMALL]
    rc, lines, _ = _run(exe, tmp_path, records)
    assert rc == 0, lines[-3:]
    runs = [ln.split() for ln in lines if ln.startswith("run ")]
    seen = {(sc.SMALL[int(i)].sample, sc.SMALL[int(i)].depth, int(path)) for _, i, path, _ in runs}
    assert seen == {(s, d, p) for s, d in sc.COMBOS for p in (0, 1, 2)}
    tiles = {sc.SMALL[int(i)].name: int(t) for _, i, _, t in runs}
    assert tiles["batch-one-tile"] == 1 and tiles["batch-two-tiles"] == 2 and tiles["batch-many-tiles-a"] > 8 and tiles["batch-one-byte"] == 1
    assert sc.case("batch-one-byte").nbytes == 1


# ---- the kernel's rules, thread by thread
CHUNKS = [sc.SHAPES, sc.COMBO + sc.LAYOUTS + sc.BATCH_EDGE, sc.VALUES]


@pytest.mark.parametrize("chunk", range(len(CHUNKS)), ids=["shapes", "layouts", "values"])
@pytest.mark.parametrize("falling", (0, 1))
def test_rules(exe, tmp_path, want, chunk, falling):
    _check_packed(exe, tmp_path, CHUNKS[chunk], want, falling, falling)


def test_every_offset(exe, tmp_path, want):
    """Every address of the destination mod 16 for cases of every path."""
    names = ["combo-f32-8-c4-CHW", "combo-u16-16-c3-CHW", "combo-u8-8-c4-HWC", "combo-f16-16-c2-HWC", "whole-bf16-8-c3-CHW", "whole-f32-16-c4-HWC",
             "xstep2-u8-8", "bottom-up-chw-f32-16", "mirror-u16-16", "broadcast-f16-8", "batch-one-byte"]
    cases = [sc.case(n) for n in names]
    for dst_mod in range(16):
        records = [c.record(4 * (dst_mod % 4), (dst_mod + 3 * k) % 16) for k, c in enumerate(cases)]
        rc, lines, data = _run(exe, tmp_path, records, dst_mod & 1)
        assert rc == 0 and lines[-1] == "ok", lines[-3:]
        assert data == b"".join(want[c.name] for c in cases) * 2, dst_mod


def test_sanitized_program(tmp_path, want):
    """The same program under AddressSanitizer and UBSan (host code, its own main): every allocation is a heap block that
    ends with its last byte."""
    _make("SANITIZE=-fsanitize=address,undefined", "SUFFIX=_san")
    san = os.path.join(BUILD, "png_source_print_san")
    _check_packed(san, tmp_path, sc.CASES, want, 2, 1)


# ---- the host checks
def _checked(exe, tmp_path, records):
    rc, lines, _ = _run(exe, tmp_path, records)
    assert rc == 0, lines
    return [ln.split(None, 2)[2] for ln in lines if ln.startswith("check ")]


def _bare(sample=sc.U8, depth=8, w=4, h=3, c=3, strides=None, order=None, offset=0, fake=1 << 40):
    ssz = sc.SAMPLE_BYTES.get(sample, 1)
    strides = strides or (w * c * ssz, c * ssz, ssz)
    case = sc.Case("bare", np.zeros(0, dtype=np.uint8), offset, strides, w, h, c, sample, depth, order or tuple(range(min(c, 4))))
    return case.record(fake=fake, with_buf=False)


def test_refusals_that_need_no_device(exe, tmp_path):
    refused = [
        (_bare(w=0), "width or height 0"), (_bare(h=0), "width or height 0"),
        (_bare(c=0, strides=(4, 1, 1), order=()), "channels"), (_bare(c=5, strides=(20, 5, 1), order=(0, 1, 2, 3)), "channels"),
        (_bare(sample=5), "unknown sample type 5"), (_bare(depth=4), "bit depth"), (_bare(depth=0), "bit depth"),
        (_bare(sample=sc.U8, depth=16), "not widened"), (_bare(sample=sc.U16, depth=8), "not narrowed"),
        (_bare(order=(0, 0, 1)), "permutation"), (_bare(order=(0, 1, 3)), "permutation"), (_bare(c=4, order=(3, 2, 1, 1)), "permutation"),
        (_bare(fake=1), "null pointer"),
        (_bare(sample=sc.F32, offset=2), "multiple of the sample's size"), (_bare(sample=sc.U16, depth=16, strides=(24, 6, 1)), "multiple"),
        (_bare(sample=sc.F16, strides=(25, 6, 2)), "multiple"), (_bare(sample=sc.F32, strides=(48, 6, 4)), "multiple"),
        (_bare(w=1 << 30, c=4, strides=(1 << 32, 4, 1), order=(0, 1, 2, 3)), "2^31"),
        # 64-bit overflow: a product, a sum, the address below 0 and above 2^64
        (_bare(h=1 << 31, strides=(1 << 62, 3, 1)), "overflows"), (_bare(h=3, w=3, strides=(1 << 62, 1 << 62, 1)), "overflows"),
        (_bare(h=3, strides=(-(1 << 62), 3, 1), fake=1 << 40), "overflows"), (_bare(h=2, strides=((1 << 62) + (1 << 61), 3, 1), fake=(1 << 63) + (1 << 62)), "overflows"),
        (_bare(h=2, strides=(-(1 << 41), 3, 1), fake=1 << 40), "overflows"),
    ]
    got = _checked(exe, tmp_path, [r for r, _ in refused])
    for line, (_, text) in zip(got, refused):
        assert not line.startswith("ok") and text in line, (line, text)
    # and what is no refusal: the largest row, a zero and a negative stride, every sample type at its depths
    fine = [_bare(w=(1 << 31) - 1, c=1, strides=((1 << 31) - 1, 1, 1), order=(0,)), _bare(strides=(0, 0, 0)), _bare(strides=(-12, 3, 1), offset=24)]
    fine += [_bare(sample=s, depth=d, strides=None) for s, d in sc.COMBOS]
    assert all(line.startswith("ok") for line in _checked(exe, tmp_path, fine))


def test_extent_for_every_sign_combination(exe, tmp_path):
    """[lo, hi) from the signs of the three strides, against the offsets the model gathers from."""
    records, want = [], []
    for sample in (sc.U8, sc.F32):
        ssz = sc.SAMPLE_BYTES[sample]
        for signs in itertools.product((1, -1), repeat=3):
            w, h, c = 5, 3, 3
            strides = (signs[0] * 40 * ssz, signs[1] * 4 * ssz, signs[2] * ssz)
            case = sc.Case("signs", np.zeros(0, dtype=np.uint8), 0, strides, w, h, c, sample, 8, (0, 1, 2))
            at = sc.offsets(case)
            records.append(case.record(fake=1 << 40, with_buf=False))
            want.append(f"ok {w * h * c} 2 {at.min()} {at.max() + ssz}")
    # a broadcast in each dimension
    for strides in ((0, 3, 1), (15, 0, 1), (15, 3, 0), (0, 0, 0)):
        case = sc.Case("zero", np.zeros(0, dtype=np.uint8), 0, strides, 5, 3, 3, sc.U8, 8, (0, 1, 2))
        at = sc.offsets(case)
        records.append(case.record(fake=1 << 40, with_buf=False))
        want.append(f"ok 45 2 {at.min()} {at.max() + 1}")
    assert _checked(exe, tmp_path, records) == want


def test_mode_and_size(exe, tmp_path):
    for c in sc.SMALL[::7]:
        line = _checked(exe, tmp_path, [c.record(0, 0)])[0].split()
        assert (int(line[1]), int(line[2])) == (c.nbytes, sc.COLORTYPE[c.channels]), c.name
