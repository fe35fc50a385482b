"""k_png_chunks, k_png_unfilter and the PNG decode entries on the device: every file of png_decode_cases.py singly and all
of them as ONE batch a mode, the files at offsets 0, 1, 3, 15 and the destinations at offsets 0, 1, 7, 15 inside one
canary-filled buffer, the results field for field those of the CPU program (tests/hostlib/png_decode_print.cc), the pixels
byte for byte the reference decoder's; the size-only mode, short capacities, malformed files beside valid ones, the forced
wide path, the second walk for many IDATs, the refusals, round trips of the library's own device-resident files, the
traffic counters.  No image is above 512 x 512."""
import os
import subprocess
import zlib

import numpy as np
import pytest
import torch

import png_decode_cases as pc
from test_gpu_inflate import FILL, Layout
from zopfli_amd import ZopfliOptions, api
from zopfli_amd._build import ROOT

pytestmark = pytest.mark.gpu

ZMX_ERR_REFUSED, ZMX_ERR_DATA = 3, 4
MODES = [(pc.OWN, "own"), (pc.RGBA8, "rgba8")]


@pytest.fixture(scope="module")
def cpu_program():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "hostlib"), "-f", "png_decode.mk"])
    exe = os.path.join(ROOT, "tests", "_build", "png_decode_print")

    def run(mode, files, capacities, hooks=None):
        hooks = hooks or [dict(force_wide=0, entry_cap=0)] * len(files)
        text = "".join(f"{mode} {'null' if cap is None else cap} 0 0 {h['force_wide']} {h['entry_cap']} {f.hex() or '-'}\n"
                       for f, cap, h in zip(files, capacities, hooks))
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        return [tuple(int(v) for v in line.split()[:16]) for line in r.stdout.splitlines()]
    return run


_REFS = {}


def reference(file, mode, capacity=None, size_only=False):
    """computed once, shared, never changed"""
    key = (file, mode, capacity, size_only)
    if key not in _REFS:
        _REFS[key] = pc.decode_ref(file, mode, capacity, size_only)
    return _REFS[key]


def _fields(result):
    """the CPU program's first sixteen fields: the result's numbers and the CRC-32 of its palette"""
    t = result.astuple()
    return t[:15] + (zlib.crc32(t[15]) & 0xffffffff,)


def _pixels(ref):
    return ref["pixels"] if ref["pixels"] is not None else b""


@pytest.mark.parametrize("mode,name", MODES, ids=["own", "rgba8"])
def test_valid_files_singly_and_as_one_batch(gpu_lib, gpu_ctx, cpu_program, mode, name):
    cases = pc.valid_cases()
    files = [c.file for c in cases]
    refs = [reference(f, mode) for f in files]
    lay = Layout(files, [r["outsize"] for r in refs])
    want = cpu_program(mode, files, lay.capacities)
    n = len(cases)
    ins, outs = [lay.stream(i) for i in range(n)], [lay.dest(i) for i in range(n)]
    # ---- ONE batch: the step on a context, then the pooled entry
    results = gpu_ctx.png_decode_device(ins, name, outs)
    for case, r, w, ref in zip(cases, results, want, refs):
        assert _fields(r) == w, case.name
        assert r.status == pc.OK and r.outsize == len(ref["pixels"]), case.name
    lay.check([r["pixels"] for r in refs])
    lay.refill()
    infos, made = api.png_decode_device_batch(ins, name, outs, lib=gpu_lib)
    assert [size for _, size in made] == [r["outsize"] for r in refs]
    assert [_fields(r) for r in infos] == want
    lay.check([r["pixels"] for r in refs])
    # ---- singly, each with the hooks its case asks for
    lay.refill()
    single = cpu_program(mode, files, lay.capacities, [c.hooks for c in cases])
    for i, case in enumerate(cases):
        r = gpu_ctx.png_decode_device([ins[i]], name, [outs[i]], force_wide=bool(case.hooks["force_wide"]),
                                      idat_capacity=case.hooks["entry_cap"] or None)[0]
        assert _fields(r) == single[i] == want[i], case.name
    lay.check([r["pixels"] for r in refs])


def test_info_and_python_shapes(gpu_lib):
    cases = [c for c in pc.planted_cases() if c.name.startswith(("palette_", "key_", "planted_ct6_bd16", "planted_ct0_bd2"))]
    d_files = [torch.from_numpy(np.frombuffer(c.file, dtype=np.uint8).copy()).cuda() for c in cases]
    infos = api.png_info_device(d_files, lib=gpu_lib)
    for case, info in zip(cases, infos):
        ref = reference(case.file, pc.OWN)
        assert (info.width, info.height, info.colortype, info.bitdepth, info.interlace, info.status) == (
            ref["width"], ref["height"], ref["colortype"], ref["bitdepth"], 0, pc.OK), case.name
        assert info.palette == ref["palette"][:4 * ref["palettesize"]], case.name
        assert info.key == ((ref["key_r"], ref["key_g"], ref["key_b"]) if ref["has_key"] else None), case.name
        assert (info.outsize_own, info.outsize_rgba8) == (ref["outsize_own"], ref["outsize_rgba8"]), case.name
    for case, d_file in zip(cases, d_files):
        for mode, name in MODES:
            ref = reference(case.file, mode)
            info, t = api.png_decode_device(d_file, name, lib=gpu_lib)
            h, w = ref["height"], ref["width"]
            if mode == pc.RGBA8:
                assert tuple(t.shape) == (h, w, 4)
            elif ref["colortype"] == 3 or ref["bitdepth"] < 8:
                assert tuple(t.shape) == (h, ref["outsize_own"] // h)
            else:
                assert tuple(t.shape) == (h, w, pc.CHANNELS[ref["colortype"]] * ref["bitdepth"] // 8)
            assert t.dtype == torch.uint8 and t.cpu().numpy().tobytes() == ref["pixels"], (case.name, name)


def test_size_only_mode_writes_nothing(gpu_lib, gpu_ctx, cpu_program):
    cases = pc.planted_cases()
    files = [c.file for c in cases]
    n = len(cases)
    for mode, name in MODES:
        refs = [reference(f, mode) for f in files]
        lay = Layout(files, [r["outsize"] for r in refs])
        ins = [lay.stream(i) for i in range(n)]
        want = cpu_program(mode, files, [None] * n)
        results = gpu_ctx.png_decode_device(ins, name, None)
        assert [_fields(r) for r in results] == want
        assert [(r.status, r.outsize) for r in results] == [(pc.OK, ref["outsize"]) for ref in refs]
        assert [_fields(r) for r in api.png_decode_size_device(ins, name, lib=gpu_lib)] == want
        lay.check([b""] * n)
        # a mixed call: every other file stored
        outs = [lay.dest(i) if i % 2 else None for i in range(n)]
        results = gpu_ctx.png_decode_device(ins, name, outs)
        assert all(r.status == pc.OK for r in results)
        lay.check([r["pixels"] if i % 2 else b"" for i, r in enumerate(refs)])


def test_capacity_one_byte_short_and_zero(gpu_lib, gpu_ctx, cpu_program):
    cases = pc.planted_cases()
    files = [c.file for c in cases]
    n = len(cases)
    mode, name = pc.RGBA8, "rgba8"
    sizes = [reference(f, mode)["outsize"] for f in files]
    caps = [s - 1 if i % 2 else 0 for i, s in enumerate(sizes)]
    lay = Layout(files, caps)
    ins, outs = [lay.stream(i) for i in range(n)], [lay.dest(i) for i in range(n)]
    want = cpu_program(mode, files, caps)
    results = gpu_ctx.png_decode_device(ins, name, outs)
    for case, r, w, size in zip(cases, results, want, sizes):
        assert _fields(r) == w and r.status == pc.CAPACITY and r.outsize == size, case.name
    assert gpu_lib.zmx_last_error_class() == ZMX_ERR_REFUSED
    assert "file 0: ZMX_PNG_DECODE_CAPACITY (12)" in gpu_ctx.error() and f"take {sizes[0]} bytes" in gpu_ctx.error()
    lay.check([b""] * n)      # nothing of an image that does not fit is stored
    with pytest.raises(api.CapacityError) as e:
        api.png_decode_device(ins[1], name, out=outs[1], lib=gpu_lib)
    assert e.value.needed == sizes[1]
    with pytest.raises(api.CapacityError) as e:
        api.png_decode_device_batch(ins[:2], name, outs[:2], lib=gpu_lib)
    assert e.value.needed == sizes[:2]
    lay.check([b""] * n)


def test_malformed_files_beside_valid_ones(gpu_lib, gpu_ctx, cpu_program):
    """Every malformed file with its status, -1, the first index in zmx_last_error(), and the valid files of the same batch
    decoded regardless."""
    good = [c.file for c in pc.planted_cases()[:3]]
    bad = pc.malformed_cases() + pc.truncation_cases()
    half = len(bad) // 2
    files = [good[0]] + [b.file for b in bad[:half]] + [good[1]] + [b.file for b in bad[half:]] + [good[2]]
    names = ["good0"] + [b.name for b in bad[:half]] + ["good1"] + [b.name for b in bad[half:]] + ["good2"]
    n = len(files)
    for mode, name in MODES:
        refs = [reference(f, mode, 4096) for f in files]
        caps = [r["outsize"] if r["status"] == pc.OK else 4096 for r in refs]
        lay = Layout(files, caps)
        ins, outs = [lay.stream(i) for i in range(n)], [lay.dest(i) for i in range(n)]
        want = cpu_program(mode, files, caps)
        results = gpu_ctx.png_decode_device(ins, name, outs)
        for nm, r, w, ref in zip(names, results, want, refs):
            assert _fields(r) == w, nm
            assert r.status == ref["status"] and (ref["detail"] == -1 or r.detail == ref["detail"]), nm
        # (an image that ends FILTER may have written the bands before the bad row: those bytes are the reference's rows)
        stored = []
        for nm, f, ref in zip(names, files, refs):
            if ref["status"] == pc.FILTER and ref["detail"] >= pc.LANES:
                rows = (ref["detail"] // pc.LANES) * pc.LANES
                whole = pc.decode_ref(_without_bad_filter(f), mode)["pixels"]
                stored.append(whole[:rows * (ref["outsize"] // ref["height"])])
            else:
                stored.append(_pixels(ref))
        lay.check(stored)
        assert gpu_lib.zmx_last_error_class() == ZMX_ERR_DATA
        lay.refill()
        with pytest.raises(api.PngDecodeError) as e:
            api.png_decode_device_batch(ins, name, outs, lib=gpu_lib)
        err = e.value
        assert err.index == 1 and err.status == refs[1]["status"]
        assert f"file 1: ZMX_PNG_DECODE_{pc.STATUS_NAMES[refs[1]['status']]} ({refs[1]['status']})" in str(err)
        assert [int(r.status) for r in err.results] == [r["status"] for r in refs]
        assert gpu_lib.zmx_last_error_class() == ZMX_ERR_DATA
        lay.check(stored)
    # the info entry: the walk and the CRCs alone
    infos = api.png_info_device(ins, lib=gpu_lib, check=False)
    for nm, info, f in zip(names, infos, files):
        ref = reference(f, pc.OWN, 4096)
        assert int(info.status) == (ref["status"] if ref["status"] <= pc.TRNS else pc.OK), nm
    with pytest.raises(api.PngDecodeError):
        api.png_info_device(ins, lib=gpu_lib)


def _without_bad_filter(f):
    """the filter_5_row_63 / _64 file with the bad type byte made 0: the rows above it are the same"""
    status, _, h, entries = pc.walk_ref(f)
    assert status == pc.OK
    (offset, length, _, _, _), = [e for e in entries if e[3] == "IDAT"]
    scan = bytearray(zlib.decompress(f[offset + 8:offset + 8 + length]))
    line = 1 + pc.linebytes_of(h["width"], h["colortype"], h["bitdepth"])
    for r in range(h["height"]):
        if scan[r * line] > 4:
            scan[r * line] = 0
    return pc.write_png(h["width"], h["height"], h["colortype"], h["bitdepth"], None, None, scanlines=bytes(scan))


def test_forced_wide_path(gpu_ctx, cpu_program):
    """every image taller than a band through the global carry rows, a launch a band, in one call"""
    cases = [c for c in pc.valid_cases() if reference(c.file, pc.OWN)["height"] > pc.LANES]
    files = [c.file for c in cases]
    n = len(cases)
    for mode, name in MODES:
        refs = [reference(f, mode) for f in files]
        lay = Layout(files, [r["outsize"] for r in refs])
        want = cpu_program(mode, files, lay.capacities, [dict(force_wide=1, entry_cap=0)] * n)
        results = gpu_ctx.png_decode_device([lay.stream(i) for i in range(n)], name, [lay.dest(i) for i in range(n)], force_wide=True)
        assert [_fields(r) for r in results] == want
        lay.check([r["pixels"] for r in refs])
    # a bad filter byte in the second band of a wide image: the lowest row, the first band written
    bad = next(b for b in pc.malformed_cases() if b.name == "filter_5_row_64")
    ref = reference(bad.file, pc.OWN, 4096)
    lay = Layout([bad.file], [ref["outsize"]])
    r = gpu_ctx.png_decode_device([lay.stream(0)], "own", [lay.dest(0)], force_wide=True)[0]
    assert (r.status, r.detail) == (pc.FILTER, 64)
    lay.check([pc.decode_ref(_without_bad_filter(bad.file), pc.OWN)["pixels"][:64 * 3]])


def test_second_walk_for_many_idats(gpu_ctx, cpu_program):
    cases = [c for c in pc.planted_cases() if c.name.startswith("idat_")]
    files = [c.file for c in cases]
    n = len(cases)
    refs = [reference(f, pc.RGBA8) for f in files]
    assert max(r["nentries"] for r in refs) > 3 * pc.ENTRIES and min(r["nentries"] for r in refs) > 3
    for cap in (1, 3, None):
        lay = Layout(files, [r["outsize"] for r in refs])
        want = cpu_program(pc.RGBA8, files, lay.capacities, [dict(force_wide=0, entry_cap=cap or 0)] * n)
        results = gpu_ctx.png_decode_device([lay.stream(i) for i in range(n)], "rgba8", [lay.dest(i) for i in range(n)], idat_capacity=cap)
        assert [_fields(r) for r in results] == want
        lay.check([r["pixels"] for r in refs])


def test_refusals(gpu_lib, gpu_ctx):
    case = pc.planted_cases()[0]
    ref = reference(case.file, pc.OWN)
    host = np.frombuffer(case.file, dtype=np.uint8).copy()
    d_file = torch.from_numpy(host).cuda()
    d_out = torch.full((2 * ref["outsize"],), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    size = len(case.file)

    def refused(text, files, outs, mode="own"):
        for call in (lambda: api.png_decode_device_batch(files, mode, outs, lib=gpu_lib), lambda: gpu_ctx.png_decode_device(files, mode, outs)):
            with pytest.raises(RuntimeError) as e:
                call()
            assert not isinstance(e.value, (api.PngDecodeError, api.CapacityError))
            assert text in str(e.value), str(e.value)
            assert gpu_lib.zmx_last_error_class() == ZMX_ERR_REFUSED
    refused("not device memory", [(host.ctypes.data, size)], [d_out])
    refused("not device memory", [d_file], [(host.ctypes.data, size)])
    refused("leaves its allocation", [(d_file.data_ptr(), 1 << 40)], [d_out])
    refused("leaves its allocation", [d_file], [(d_out.data_ptr(), 1 << 40)])
    both = torch.zeros(size + 2 * ref["outsize"], dtype=torch.uint8, device="cuda:0")
    both[:size] = d_file
    torch.cuda.synchronize()
    refused("destination 1 overlaps input 0", [both[:size], d_file], [d_out[:ref["outsize"]], both[size - 1:]])
    refused("destination 1 overlaps destination 0", [d_file, d_file], [d_out[:ref["outsize"]], d_out[ref["outsize"] - 1:]])
    refused("unknown mode 7", [d_file], [d_out], mode=7)
    assert bool((d_out == FILL).all()), "a refused call wrote"
    # a header whose scanlines cannot be held: refused after the walk, before any stream is read
    huge = bytearray(pc.write_png(1, 1, 6, 16, [bytes(8)], [0]))
    huge[16:24] = (0x7fffffff).to_bytes(4, "big") * 2
    huge[29:33] = (zlib.crc32(bytes(huge[12:29])) & 0xffffffff).to_bytes(4, "big")
    d_huge = torch.from_numpy(np.frombuffer(bytes(huge), dtype=np.uint8).copy()).cuda()
    refused("scanlines take 2^40 bytes or more", [d_huge], [d_out])
    # n = 0 returns at once
    assert api.png_decode_device_batch([], "own", [], lib=gpu_lib) == ([], []) and gpu_ctx.png_decode_device([], "own", []) == []
    assert api.png_info_device([], lib=gpu_lib) == []
    # ... and the call that all these refusals were of goes through
    info, t = api.png_decode_device(d_file, "own", out=d_out, lib=gpu_lib)
    assert t.cpu().numpy().tobytes() == ref["pixels"]


# ---- round trips of the library's own device-resident files: no reference involved
def _smooth(w, h, channels, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w * channels]
    return ((x // channels * 3 + y * 2 + (x % channels) * 40 + rng.integers(-3, 4, size=(h, w * channels))) & 255).astype(np.uint8).reshape(h, w, channels)


def _encode_own_again(info, pixels, strategy, options, lib):
    """the file of a decoded OWN image, its colour type kept: the index entry for palette images and grey below 8 bits"""
    w, h, ct, bd = int(info.width), int(info.height), int(info.colortype), int(info.bitdepth)
    if ct == 3 or bd < 8:
        palette = np.frombuffer(info.palette, dtype=np.uint8).reshape(-1, 4) if ct == 3 else None
        d_file = torch.empty(api.png_index_bound(w, h, ct, bd, lib=lib), dtype=torch.uint8, device="cuda:0")
        size = api.png_index_encode_device_out((pixels, w, h, ct, bd, palette), d_file, strategy, options, lib=lib)
    else:
        d_file = torch.empty(api.png_bound(w, h, ct, bd, lib=lib), dtype=torch.uint8, device="cuda:0")
        size = api.png_encode_device_out((pixels.data_ptr(), w, h, ct, bd), d_file, strategy, options, lib=lib)
    return d_file[:size]


@pytest.mark.parametrize("strategy", ["0", "e", "4"])
def test_round_trip_of_png_encode_device_out(gpu_lib, strategy):
    for (w, h, channels, ct) in [(129, 65, 4, 6), (65, 129, 3, 2), (7, 64, 1, 0), (64, 63, 2, 4)]:
        img = torch.from_numpy(_smooth(w, h, channels, 5)).cuda()
        d_file = torch.empty(api.png_bound(w, h, ct, 8, lib=gpu_lib), dtype=torch.uint8, device="cuda:0")
        size = api.png_encode_device_out(img, d_file, strategy, ZopfliOptions(2), lib=gpu_lib)
        info, back = api.png_decode_device(d_file[:size], "own", lib=gpu_lib)
        assert (info.width, info.height, info.colortype, info.bitdepth) == (w, h, ct, 8)
        assert torch.equal(back.reshape(h, w, channels), img), (w, h, ct)
        again = _encode_own_again(info, back, strategy, ZopfliOptions(2), gpu_lib)
        assert torch.equal(again, d_file[:size]), (w, h, ct)
        if ct == 6:
            assert torch.equal(api.png_decode_device(d_file[:size], "rgba8", lib=gpu_lib)[1], img)


@pytest.mark.parametrize("strategy", ["0", "e", "4"])
def test_round_trip_of_png_optimize_device_out(gpu_lib, strategy):
    """an RGBA8 image of few colours becomes a palette file; its RGBA8 decode is the image, its OWN decode encodes to the same
    file again"""
    rng = np.random.default_rng(11)
    w, h = 65, 65
    colours = rng.integers(0, 256, size=(12, 4), dtype=np.uint8)
    colours[:3, 3] = (0, 128, 255)
    colours[0, :3] = 0      # (one fully transparent colour, already black: nothing for the encoder to rewrite)
    index = (np.add.outer(np.arange(h), np.arange(w)) // 3 % 12).astype(np.int64)
    img = torch.from_numpy(colours[index]).cuda()
    d_file = torch.empty(api.png_bound(w, h, 6, 8, lib=gpu_lib), dtype=torch.uint8, device="cuda:0")
    size = api.png_optimize_device_out(img, d_file, strategy, ZopfliOptions(2), lib=gpu_lib)
    info, own = api.png_decode_device(d_file[:size], "own", lib=gpu_lib)
    assert (info.colortype, info.bitdepth, info.palettesize) == (3, 4, 12)
    assert tuple(own.shape) == (h, (w * 4 + 7) // 8)
    assert torch.equal(api.png_decode_device(d_file[:size], "rgba8", lib=gpu_lib)[1], img)
    again = _encode_own_again(info, own, strategy, ZopfliOptions(2), gpu_lib)
    assert torch.equal(again, d_file[:size])


@pytest.mark.parametrize("strategy", ["0", "e", "4"])
def test_round_trip_of_png_index_encode_device_out(gpu_lib, strategy):
    rng = np.random.default_rng(13)
    for (w, h, ct, bd, entries) in [(129, 65, 3, 8, 200), (65, 64, 3, 2, 4), (63, 65, 0, 4, 0), (9, 129, 0, 1, 0)]:
        line = (w * bd + 7) // 8
        rows = rng.integers(0, 256, size=(h, line), dtype=np.uint8)
        if bd < 8 and (w * bd) % 8:
            rows[:, -1] &= (0xff << (8 - (w * bd) % 8)) & 0xff
        if ct == 3 and bd == 8:
            rows %= entries
        palette = rng.integers(0, 256, size=(entries, 4), dtype=np.uint8) if ct == 3 else None
        d_rows = torch.from_numpy(rows).cuda()
        d_file = torch.empty(api.png_index_bound(w, h, ct, bd, lib=gpu_lib), dtype=torch.uint8, device="cuda:0")
        size = api.png_index_encode_device_out((d_rows, w, h, ct, bd, palette), d_file, strategy, ZopfliOptions(2), lib=gpu_lib)
        info, back = api.png_decode_device(d_file[:size], "own", lib=gpu_lib)
        assert (info.width, info.height, info.colortype, info.bitdepth) == (w, h, ct, bd)
        assert torch.equal(back, d_rows), (w, h, ct, bd)
        again = _encode_own_again(info, back, strategy, ZopfliOptions(2), gpu_lib)
        assert torch.equal(again, d_file[:size]), (w, h, ct, bd)


def test_round_trip_out_of_a_packed_arena(gpu_lib):
    imgs = [torch.from_numpy(_smooth(64 - i, 33 + 2 * i, 4, i)).cuda() for i in range(16)]
    arena = torch.empty(api.png_batch_bound(imgs, 16, lib=gpu_lib), dtype=torch.uint8, device="cuda:0")
    offsets, sizes = api.png_encode_device_batch_packed(imgs, arena, 16, "e", ZopfliOptions(2), lib=gpu_lib)
    files = [(arena.data_ptr() + o, s) for o, s in zip(offsets, sizes)]
    for name in ("own", "rgba8"):
        infos, backs = api.png_decode_device_batch(files, name, lib=gpu_lib)
        for img, info, back in zip(imgs, infos, backs):
            assert (info.colortype, info.bitdepth) == (6, 8) and torch.equal(back, img)
    traffic_in, traffic_out = api.last_input_traffic(gpu_lib), api.last_output_traffic(gpu_lib)
    assert traffic_in == [0, 0, 0] and traffic_out[0] == 0 and traffic_out[1] == 0      # no byte of a file or of a pixel crosses


def test_round_trip_of_512_x_512(gpu_lib):
    img = torch.from_numpy(_smooth(512, 512, 4, 17)).cuda()
    d_file = torch.empty(api.png_bound(512, 512, 6, 8, lib=gpu_lib), dtype=torch.uint8, device="cuda:0")
    size = api.png_encode_device_out(img, d_file, "e", ZopfliOptions(1), lib=gpu_lib)
    for name in ("own", "rgba8"):
        info, back = api.png_decode_device(d_file[:size], name, lib=gpu_lib)
        assert torch.equal(back, img)
