"""k_png_unpack and the sink entries on the device.  Context.png_unpack_device is held byte for byte to the numpy model of
tests/png_sink_cases.py on every case and sink — a launch of its own each, and all of them as ONE batch launch —, the
guard and gap bytes and the inputs as they were; png_decode_device_batch(outs=sinks) and png_decode_tensors are held on
the case files to the model's samples and, where the target is 8-bit, to the torch chain on the existing rgba8 output;
mixed batches (a wrong size, a malformed file, valid ones; the forced wide path), the round trip through the encoder, the
refusals that need a device, and the existing entries with today's arguments.  No image is above 70 x 70 but the three
rows that stand on a tile's end."""
import os
import subprocess

import numpy as np
import pytest
import torch

import png_decode_cases as pc
import png_sink_cases as sk
from zopfli_amd import ZopfliOptions, api
from zopfli_amd._build import ROOT

pytestmark = pytest.mark.gpu

ZMX_ERR_REFUSED, ZMX_ERR_DATA = 3, 4
DTYPES = {sk.U8: torch.uint8, sk.U16: torch.uint16, sk.F16: torch.float16, sk.BF16: torch.bfloat16, sk.F32: torch.float32}


@pytest.fixture(scope="module")
def tile():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "hostlib"), "-f", "png_sink.mk"])
    return int(subprocess.check_output([os.path.join(ROOT, "tests", "_build", "png_sink_print"), "constants"], text=True).split()[0])


def _mode_result(m):
    """the zmx_png_decode_result that says what own-mode pixels are"""
    r = api.PngDecodeResult()
    for key in ("width", "height", "colortype", "bitdepth", "palettesize", "has_key", "key_r", "key_g", "key_b"):
        setattr(r, key, m[key])
    r.outsize = r.outsize_own = pc.linebytes_of(m["width"], m["colortype"], m["bitdepth"]) * m["height"]
    r.outsize_rgba8 = 4 * m["width"] * m["height"]
    r.palette_bytes[:] = list(m["palette"])
    return r


class Arena:
    """Every case's allocation in ONE device buffer of FILL bytes, case k's at a 16-byte boundary plus 4 * (k % 4); the
    model's allocations side by side to compare with; the inputs (`blobs`: files, or own-mode pixels) in ONE other tensor, at
    every byte alignment."""

    def __init__(self, cases, blobs):
        self.cases = cases
        self.at, cur = [], sk.GUARD
        for k, c in enumerate(cases):
            cur += (4 * (k % 4) + 16 - cur % 16) % 16
            self.at.append(cur)
            cur += c.sink.buflen
        self.size = cur + sk.GUARD
        self.dev = torch.full((self.size,), sk.FILL, dtype=torch.uint8, device="cuda:0")
        self.in_at, cur = [], 0
        for k, b in enumerate(blobs):
            cur += (k % 16 + 16 - cur % 16) % 16
            self.in_at.append(cur)
            cur += len(b)
        host = np.zeros(cur + 16, dtype=np.uint8)
        for at, b in zip(self.in_at, blobs):
            host[at:at + len(b)] = np.frombuffer(b, dtype=np.uint8)
        self.in_host = host
        self.in_dev = torch.from_numpy(host).cuda()
        self.blobs = blobs
        torch.cuda.synchronize()

    def sink(self, k):
        s = self.cases[k].sink
        return api.PngSink((self.dev.data_ptr() + self.at[k] + s.offset, s.sy, s.sx, s.sc, s.width, s.height, s.channels, s.sample, s.depth, s.order))

    def input(self, k):
        return (self.in_dev.data_ptr() + self.in_at[k], len(self.blobs[k]))

    def expected(self, stored=None):
        """the arena with the model's samples of every case (`stored`: of those cases alone) scattered into it"""
        want = np.full(self.size, sk.FILL, dtype=np.uint8)
        for k, c in enumerate(self.cases):
            if stored is None or k in stored:
                want[self.at[k]:self.at[k] + c.sink.buflen] = c.sink.expected(*sk.mode_of(c.file))
        return want

    def check(self, stored=None):
        torch.cuda.synchronize()
        got, want = self.dev.cpu().numpy(), self.expected(stored)
        if not np.array_equal(got, want):
            at = int(np.flatnonzero(got != want)[0])
            k = max(i for i in range(len(self.at)) if self.at[i] <= at) if at >= self.at[0] else -1
            raise AssertionError(f"arena byte {at} differs: case {self.cases[k].name if k >= 0 else 'the guard'}, byte {at - self.at[max(k, 0)]} of its allocation")
        assert np.array_equal(self.in_dev.cpu().numpy(), self.in_host), "an input was written"

    def refill(self):
        self.dev.fill_(sk.FILL)
        torch.cuda.synchronize()


# ---- k_png_unpack
def test_unpack_singly_and_as_one_batch(gpu_ctx, tile):
    cases = sk.cases(tile)
    modes = [_mode_result(sk.mode_of(c.file)[0]) for c in cases]
    arena = Arena(cases, [sk.mode_of(c.file)[1] for c in cases])
    n = len(cases)
    sinks, owns = [arena.sink(k) for k in range(n)], [arena.input(k) for k in range(n)]
    gpu_ctx.png_unpack_device(modes, owns, sinks)          # ONE launch
    arena.check()
    arena.refill()
    for k in range(n):                                     # a launch each
        gpu_ctx.png_unpack_device([modes[k]], [owns[k]], [sinks[k]])
    arena.check()
    gpu_ctx.png_unpack_device([], [], [])                  # n = 0


def test_unpack_into_one_nchw_tensor(gpu_ctx):
    """five unlike images into ONE (N, C, H, W) tensor and ONE (N, H, W, C) tensor: the images' samples lie side by side"""
    files = [f for f in sk.extra_files() if f.name.startswith("pair_")][3:8]
    for (sample, depth), layout in (((sk.F32, 8), "NCHW"), ((sk.U16, 16), "NHWC"), ((sk.BF16, 16), "NCHW")):
        m0, _ = sk.mode_of(files[0].file)
        w, h = m0["width"], m0["height"]
        batch = torch.zeros((5, 3, h, w) if layout == "NCHW" else (5, h, w, 3), dtype=DTYPES[sample], device="cuda:0")
        owns = [torch.from_numpy(np.frombuffer(sk.mode_of(f.file)[1], dtype=np.uint8).copy()).cuda() for f in files]
        gpu_ctx.png_unpack_device([_mode_result(sk.mode_of(f.file)[0]) for f in files], owns, api.png_sinks(batch, layout, bitdepth=depth))
        got = batch.cpu().view(torch.uint8).numpy().reshape(5, -1)
        for i, f in enumerate(files):
            v = sk.values(*sk.mode_of(f.file), 3, depth)
            want = sk.samples(v if layout == "NHWC" else v.transpose(2, 0, 1), sample, depth)
            assert np.array_equal(got[i], want.reshape(-1)), (f.name, layout)


# ---- the decode entries
def _chain(rgba8, sink):
    """The torch chain on the rgba8 tensor (H, W, 4) the existing entry wrote: the samples' bytes, (H, W, C, ssz).  The
    arithmetic runs where torch's div IS a division: on the host.  (On the device torch divides a tensor by a Python scalar
    by multiplying with the fp32 reciprocal — one unit in the last place off the division in 126 of the 256 byte values, as
    test_float_sinks_against_the_torch_chain prints —; the value rule of include/zopfli_amd.h asks for the division.)"""
    rgba8 = rgba8.cpu()
    t = {1: rgba8[..., :1], 2: rgba8[..., [0, 3]], 3: rgba8[..., :3], 4: rgba8}[sink.channels]
    if sink.sample != sk.U8:
        t = t.float().div(255).to(DTYPES[sink.sample])
    return t.contiguous().view(torch.uint8).numpy().reshape(sink.height, sink.width, sink.channels, sink.ssz)


def test_decode_into_sinks_is_the_model_and_the_torch_chain(gpu_lib, gpu_ctx, tile):
    cases = sk.cases(tile)
    arena = Arena(cases, [c.file for c in cases])
    n = len(cases)
    sinks, files = [arena.sink(k) for k in range(n)], [arena.input(k) for k in range(n)]
    infos, tensors = api.png_decode_device_batch(files, outs=sinks, lib=gpu_lib)
    assert all(r.status == pc.OK for r in infos) and tensors == [None] * n
    assert api.last_input_traffic(gpu_lib)[0] == 0 and api.last_output_traffic(gpu_lib)[0] == 0
    arena.check()
    got = arena.dev.cpu().numpy()
    # the torch chain on the existing rgba8 output, where the target's samples are 8-bit: a selection of channels
    eight = [k for k in range(n) if cases[k].sink.sample == sk.U8]
    _, rgba = api.png_decode_device_batch([files[k] for k in eight], "rgba8", lib=gpu_lib)
    for k, t in zip(eight, rgba):
        s = cases[k].sink
        assert np.array_equal(got[arena.at[k]:arena.at[k] + s.buflen][s.sample_bytes()], _chain(t, s)), cases[k].name
    # the step on a context, and one file at a time through the single entry
    arena.refill()
    results = gpu_ctx.png_decode_device(files, outs=sinks)
    assert [int(r.status) for r in results] == [pc.OK] * n
    arena.check()
    arena.refill()
    some = list(range(0, n, 9))
    for k in some:
        info, _ = api.png_decode_device(files[k], out=sinks[k], lib=gpu_lib)
        assert (info.width, info.height) == (cases[k].sink.width, cases[k].sink.height)
    arena.check(set(some))


def test_decode_tensors(gpu_lib):
    files = [f for f in sk.extra_files() if f.name.startswith("pair_")]
    d_files = [torch.from_numpy(np.frombuffer(f.file, dtype=np.uint8).copy()).cuda() for f in files]
    for dtype, sample, channels, layout, bitdepth in ((None, sk.F32, 3, "NCHW", None), (torch.uint16, sk.U16, 4, "NHWC", None),
                                                      (torch.float16, sk.F16, 1, "NCHW", 16), (torch.uint8, sk.U8, 2, "NHWC", None)):
        infos, batch = api.png_decode_tensors(d_files, dtype, channels, layout, bitdepth, lib=gpu_lib)
        depth = bitdepth or (16 if sample == sk.U16 else 8)
        assert batch.dtype == DTYPES[sample] and tuple(batch.shape) == ((15, channels, 5, 13) if layout == "NCHW" else (15, 5, 13, channels))
        got = batch.cpu().view(torch.uint8).numpy().reshape(15, -1)
        for i, f in enumerate(files):
            v = sk.values(*sk.mode_of(f.file), channels, depth)
            want = sk.samples(v if layout == "NHWC" else v.transpose(2, 0, 1), sample, depth)
            assert np.array_equal(got[i], want.reshape(-1)), (f.name, layout)
            assert (infos[i].colortype, infos[i].bitdepth) == (sk.mode_of(f.file)[0]["colortype"], sk.mode_of(f.file)[0]["bitdepth"])
    _, batch = api.png_decode_tensors(d_files, lib=gpu_lib)
    other = torch.from_numpy(np.frombuffer(sk.extra_files()[-1].file, dtype=np.uint8).copy()).cuda()
    with pytest.raises(ValueError, match="file 2 is 9 x 5"):
        api.png_decode_tensors(d_files[:2] + [other], lib=gpu_lib)
    with pytest.raises(ValueError, match="not both"):
        api.png_decode_device_batch(d_files[:2], outs=[api.PngSink(batch[0], "CHW"), batch[1]], lib=gpu_lib)


@pytest.mark.parametrize("sample", (sk.F16, sk.BF16, sk.F32), ids=["f16", "bf16", "f32"])
def test_float_sinks_against_the_torch_chain(gpu_lib, tile, sample):
    """The second reference for the float targets of 8-bit values: `.float().div(255)` applied to the existing rgba8 output
    differs from the sink in no value, for every float case.  The chain's arithmetic runs on the host (_chain), where
    torch's div is the one correctly rounded fp32 division the value rule names.  What torch's chain gives ON THE DEVICE is
    printed, not asserted: there a div by a Python scalar is a multiply by the fp32 reciprocal — measured on an MI355X, it
    differs from the division in 126 of the 256 byte values (one unit in the last place) and from v * fl32(1 / 255) in
    none, so 119 of the 128 float32 cases differ from a device-side chain in some value; rounded to float16 or bfloat16
    the two agree everywhere."""
    cases = [c for c in sk.cases(tile) if c.sink.depth == 8 and c.sink.sample == sample]
    arena = Arena(cases, [c.file for c in cases])
    n = len(cases)
    files = [arena.input(k) for k in range(n)]
    api.png_decode_device_batch(files, outs=[arena.sink(k) for k in range(n)], lib=gpu_lib)
    arena.check()
    got = arena.dev.cpu().numpy()
    _, rgba = api.png_decode_device_batch(files, "rgba8", lib=gpu_lib)
    v = torch.arange(256, dtype=torch.uint8, device="cuda:0")
    chain256 = v.float().div(255).cpu().numpy()
    exact = np.arange(256, dtype=np.float32) / np.float32(255)
    recip = np.arange(256, dtype=np.float32) * (np.float32(1) / np.float32(255))
    print("torch's .float().div(255) of the 256 byte values on the device: differs from the fp32 division in", int((chain256 != exact).sum()),
          "values, from the multiply by the fp32 reciprocal in", int((chain256 != recip).sum()))
    differing = {}
    for k, t in enumerate(rgba):
        s = cases[k].sink
        mine, theirs = got[arena.at[k]:arena.at[k] + s.buflen][s.sample_bytes()], _chain(t, s)
        if not np.array_equal(mine, theirs):
            differing[cases[k].name] = int((mine != theirs).any(axis=-1).sum())
    print(len(differing), "of", n, sk.SAMPLE_NAMES[sample], "cases differ from the chain")
    assert not differing, (len(differing), "of", n)
    assert np.array_equal(v.cpu().float().div(255).numpy(), exact), "torch's div on the host is the fp32 division"


@pytest.mark.parametrize("force_wide", (False, True))
def test_mixed_batches(gpu_lib, gpu_ctx, force_wide):
    """a file of the wrong size, a malformed file and valid files in one call"""
    pair = {f.name: f for f in sk.extra_files()}
    good = [pair["pair_ct6_bd8_13x5"], pair["pair_ct3_bd4_13x5"], pair["pair_ct2_bd16_13x5"]]
    wrong_size = pair["low_bytes_ct6"]                                        # 9 x 5
    bad = next(b for b in pc.malformed_cases() if b.name == "crc_IDAT")
    files = [good[0].file, wrong_size.file, bad.file, good[1].file, good[2].file]
    sinks = [sk.contiguous(13, 5, 3, sk.F32, 8, "CHW"), sk.contiguous(13, 5, 4, sk.U8, 8, "HWC"), sk.contiguous(5, 3, 3, sk.U8, 8, "HWC"),
             sk.contiguous(13, 5, 4, sk.U16, 16, "HWC"), sk.contiguous(13, 5, 2, sk.BF16, 16, "CHW")]
    cases = [sk.Case(str(k), f, s) for k, (f, s) in enumerate(zip(files, sinks))]
    arena = Arena(cases, files)
    ins, outs = [arena.input(k) for k in range(5)], [arena.sink(k) for k in range(5)]
    results = gpu_ctx.png_decode_device(ins, outs=outs, force_wide=force_wide)
    assert [int(r.status) for r in results] == [pc.OK, sk.SHAPE, pc.CRC, pc.OK, pc.OK]
    assert (results[1].width, results[1].height, results[1].colortype, results[1].bitdepth) == (9, 5, 6, 16)
    assert "file 1: ZMX_PNG_DECODE_SHAPE (13)" in gpu_ctx.error() and gpu_lib.zmx_last_error_class() == ZMX_ERR_DATA
    arena.check({0, 3, 4})                                                    # (the two others' sinks as they were)
    arena.refill()
    with pytest.raises(api.PngDecodeError) as e:
        api.png_decode_device_batch(ins, outs=outs, lib=gpu_lib)
    assert e.value.index == 1 and e.value.status == sk.SHAPE and [int(r.status) for r in e.value.results] == [0, sk.SHAPE, pc.CRC, 0, 0]
    assert "file 1: ZMX_PNG_DECODE_SHAPE (13)" in str(e.value) and gpu_lib.zmx_last_error_class() == ZMX_ERR_DATA
    assert api.last_input_traffic(gpu_lib)[0] == 0 and api.last_output_traffic(gpu_lib)[0] == 0
    arena.check({0, 3, 4})


def test_round_trip_through_the_encoder(gpu_lib):
    """decode into float32 CHW sinks, encode PngSources over the same tensors, decode `own`: the original's own pixels"""
    options = ZopfliOptions(2)
    for f in sk.extra_files():
        m, own = sk.mode_of(f.file)
        if not f.name.startswith(("pair_", "low_bytes")) or m["colortype"] == 3 or m["bitdepth"] < 8:
            continue
        d_file = torch.from_numpy(np.frombuffer(f.file, dtype=np.uint8).copy()).cuda()
        t = torch.zeros((pc.CHANNELS[m["colortype"]], m["height"], m["width"]), dtype=torch.float32, device="cuda:0")
        api.png_decode_device(d_file, out=api.PngSink(t, "CHW", bitdepth=m["bitdepth"]), lib=gpu_lib)
        again = api.png_encode_device(api.PngSource(t, "CHW", bitdepth=m["bitdepth"]), "e", options, None, gpu_lib)
        d_again = torch.from_numpy(np.frombuffer(again, dtype=np.uint8).copy()).cuda()
        info, px = api.png_decode_device(d_again, "own", lib=gpu_lib)
        assert (info.colortype, info.bitdepth) == (m["colortype"], m["bitdepth"]) and px.cpu().numpy().tobytes() == own, f.name


# ---- refusals
def test_refusals(gpu_lib, gpu_ctx):
    f = next(x for x in sk.extra_files() if x.name == "pair_ct6_bd8_13x5")
    m, own = sk.mode_of(f.file)
    d_file = torch.from_numpy(np.frombuffer(f.file, dtype=np.uint8).copy()).cuda()
    d_own = torch.from_numpy(np.frombuffer(own, dtype=np.uint8).copy()).cuda()
    dst = torch.full((3 * 4096,), sk.FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()

    def sink(ptr, strides=(52, 4, 1), w=13, h=5, c=4, sample=sk.U8, depth=8, order=(0, 1, 2, 3)):
        return api.PngSink((ptr, *strides, w, h, c, sample, depth, order))

    good = sink(dst.data_ptr())
    mode = _mode_result(m)

    def refused(sinks, text, files=None, owns=None):
        k = len(sinks)
        for call in (lambda: gpu_ctx.png_unpack_device([mode] * k, owns or [d_own] * k, sinks),
                     lambda: gpu_ctx.png_decode_device(files or [d_file] * k, outs=sinks),
                     lambda: api.png_decode_device_batch(files or [d_file] * k, outs=sinks, lib=gpu_lib)):
            with pytest.raises(RuntimeError) as e:
                call()
            assert text in str(e.value) and not isinstance(e.value, api.PngDecodeError), str(e.value)
            assert gpu_lib.zmx_last_error_class() == ZMX_ERR_REFUSED

    # every sentence of the list that needs no device, through the entries, with the index in the message
    for s, text in sk.refusals():
        try:
            bad = api.PngSink(((1 << 40) + s.offset, s.sy, s.sx, s.sc, s.width, s.height, s.channels, s.sample, s.depth, s.order))
        except ValueError:
            continue            # (five channels: PngSink itself says so; tests/test_cpu_png_sink_cases.py holds the library to it)
        refused([good, bad], "sink 1: ")
        with pytest.raises(RuntimeError, match=text):
            api.png_sink_check(bad, gpu_lib)
    api.png_sink_check(good, gpu_lib)
    # foreign memory, an extent that leaves its allocation (rows a GiB apart, running down from the tensor)
    host_mem = np.zeros(4096, dtype=np.uint8)
    refused([good, sink(host_mem.ctypes.data)], "sink 1: the extent")
    refused([sink(dst.data_ptr(), strides=(-(1 << 30), 4, 1)), sink(dst.data_ptr() + 4096)], "sink 0: the extent")
    # a sink over another sink (in the gap of its pitch, where no sample lies), over a file, over the input pixels
    pitched = sink(dst.data_ptr(), strides=(128, 4, 1))
    refused([pitched, sink(dst.data_ptr() + 64, strides=(128, 4, 1))], "sink 1: its extent overlaps that of sink 0")
    both = torch.full((8192,), sk.FILL, dtype=torch.uint8, device="cuda:0")
    both[100:100 + len(f.file)] = d_file
    both[4096:4096 + len(own)] = d_own
    torch.cuda.synchronize()
    over_file = sink(both.data_ptr(), strides=(128, 4, 1))
    for call in (lambda: gpu_ctx.png_decode_device([(both.data_ptr() + 100, len(f.file))], outs=[over_file]),
                 lambda: api.png_decode_device_batch([(both.data_ptr() + 100, len(f.file))], outs=[over_file], lib=gpu_lib)):
        with pytest.raises(RuntimeError, match="sink 0: its extent overlaps file 0"):
            call()
        assert gpu_lib.zmx_last_error_class() == ZMX_ERR_REFUSED
    with pytest.raises(RuntimeError, match="sink 0 overlaps its pixels"):
        gpu_ctx.png_unpack_device([mode], [(both.data_ptr() + 4096, len(own))], [sink(both.data_ptr() + 4000, strides=(128, 4, 1))])
    # what zmx_png_unpack_device refuses of a mode: not OK, no legal pair, another size, pixels in host memory
    for change, text in ((dict(status=pc.CRC), "not ZMX_PNG_DECODE_OK"), (dict(colortype=2, bitdepth=4), "no PNG mode"), (dict(width=12), "the sink is 13 x 5")):
        other = _mode_result(m)
        for key, v in change.items():
            setattr(other, key, v)
        with pytest.raises(RuntimeError, match="image 1: .*" + text):
            gpu_ctx.png_unpack_device([mode, other], [d_own, d_own], [good, sink(dst.data_ptr() + 4096)])
        assert gpu_lib.zmx_last_error_class() == ZMX_ERR_REFUSED
    with pytest.raises(RuntimeError, match="image 0: the pixels"):
        gpu_ctx.png_unpack_device([mode], [(host_mem.ctypes.data, len(own))], [good])
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == sk.FILL).all() and (both[:100].cpu().numpy() == sk.FILL).all(), "a refused call wrote"


def test_existing_entries_with_todays_arguments(gpu_lib, gpu_ctx):
    """mode and tensors as before: today's outputs, on a handful of cases"""
    cases = pc.planted_cases()[::9]
    d_files = [torch.from_numpy(np.frombuffer(c.file, dtype=np.uint8).copy()).cuda() for c in cases]
    for mode, name in ((pc.OWN, "own"), (pc.RGBA8, "rgba8")):
        infos, made = api.png_decode_device_batch(d_files, name, lib=gpu_lib)
        for c, info, t in zip(cases, infos, made):
            ref = pc.decode_ref(c.file, mode)
            assert info.status == pc.OK and t.dtype == torch.uint8 and t.cpu().numpy().tobytes() == ref["pixels"], (c.name, name)
        outs = [torch.zeros(int(i.outsize), dtype=torch.uint8, device="cuda:0") for i in infos]
        results = gpu_ctx.png_decode_device(d_files, name, outs)
        assert [o.cpu().numpy().tobytes() for o in outs] == [pc.decode_ref(c.file, mode)["pixels"] for c in cases]
        assert [r.astuple() for r in results] == [i.astuple() for i in infos]
        info, t = api.png_decode_device(d_files[0], name, lib=gpu_lib)
        assert t.cpu().numpy().tobytes() == pc.decode_ref(cases[0].file, mode)["pixels"]
