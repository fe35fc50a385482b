"""k_inflate and the inflate entries on the device: every stream of inflate_cases.py singly and as one batch a format, at
input offsets 0, 1, 3, 15 and output offsets 0, 1, 7, 15 inside one canary-filled buffer, the results field for field those
of the CPU program (tests/hostlib/inflate_print.cc); the size-only mode, short capacities, the malformed streams beside
valid ones, the trailer comparison, round trips of the library's own device-resident output, the refusals.  No stream is
above 4 MB."""
import ctypes
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest
import torch

import inflate_cases as ic
from zopfli_amd import ZopfliOptions, api, generate
from zopfli_amd._build import ROOT

pytestmark = pytest.mark.gpu

ZMX_ERR_REFUSED, ZMX_ERR_DATA = 3, 4
FILL = 0xa5
GUARD = 32
IN_SHIFTS, OUT_SHIFTS = (0, 1, 3, 15), (0, 1, 7, 15)


def _align(x, a=16):
    return (x + a - 1) // a * a


class Layout:
    """Streams in one device buffer at 16-byte boundaries plus their shifts, destinations in one canary-filled buffer with
    GUARD bytes between them."""

    def __init__(self, streams, capacities):
        self.in_at, self.out_at, self.capacities = [], [], list(capacities)
        host, at = bytearray(), 0
        for i, s in enumerate(streams):
            at = _align(len(host)) + IN_SHIFTS[i % 4]
            host += bytes(at - len(host)) + s
            self.in_at.append(at)
        at = 0
        for i, cap in enumerate(capacities):
            at = _align(at + GUARD) + OUT_SHIFTS[(i // 4) % 4]
            self.out_at.append(at)
            at += cap
        self.sizes = [len(s) for s in streams]
        self.d_in = torch.from_numpy(np.frombuffer(bytes(host) + b"\x00", dtype=np.uint8).copy()).cuda()
        self.d_out = torch.full((at + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        assert self.d_in.data_ptr() % 16 == 0 and self.d_out.data_ptr() % 16 == 0

    def stream(self, i):
        return (self.d_in.data_ptr() + self.in_at[i], self.sizes[i])

    def dest(self, i):
        return (self.d_out.data_ptr() + self.out_at[i], self.capacities[i])

    def refill(self):
        self.d_out.fill_(FILL)
        torch.cuda.synchronize()

    def check(self, expected):
        """destination i holds expected[i] (up to its capacity) and every other byte of the buffer is the canary's"""
        host = self.d_out.cpu().numpy()
        want = np.full(host.shape, FILL, dtype=np.uint8)
        for at, cap, exp in zip(self.out_at, self.capacities, expected):
            n = min(cap, len(exp))
            want[at:at + n] = np.frombuffer(exp[:n], dtype=np.uint8)
        bad = np.nonzero(host != want)[0]
        assert bad.size == 0, f"byte {int(bad[0])} of the destinations' buffer differs ({bad.size} in all)"


@pytest.fixture(scope="module")
def cpu_program():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "hostlib"), "-f", "inflate.mk"])
    exe = os.path.join(ROOT, "tests", "_build", "inflate_print")

    def run(fmt, streams, capacities):
        text = "".join(f"{fmt} {'null' if cap is None else cap} 0 0 {s.hex() or '-'}\n" for s, cap in zip(streams, capacities))
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        return [tuple(int(v) for v in line.split()[:6]) for line in r.stdout.splitlines()]
    return run


def _fields(result):
    """(status, outsize, consumed, block, stored_check, stored_isize): the CPU program's order"""
    return (int(result.status), int(result.outsize), int(result.consumed), int(result.block), int(result.stored_check), int(result.stored_isize))


def _by_format(cases):
    return [(fmt, [c for c in cases if c.fmt == fmt]) for fmt in (ic.GZIP, ic.ZLIB, ic.DEFLATE)]


@pytest.mark.parametrize("fmt,cases", _by_format(ic.valid_cases()), ids=["gzip", "zlib", "deflate"])
def test_valid_streams_singly_and_as_one_batch(gpu_lib, gpu_ctx, cpu_program, fmt, cases):
    streams, expected = [c.stream for c in cases], [c.expect for c in cases]
    lay = Layout(streams, [len(e) for e in expected])
    want = cpu_program(fmt, streams, lay.capacities)
    n = len(cases)
    # ---- one launch for all of them: the step, then the pooled entry with its checksums
    results = gpu_ctx.inflate_device([lay.stream(i) for i in range(n)], fmt, [lay.dest(i) for i in range(n)])
    for case, r, w in zip(cases, results, want):
        assert _fields(r) == w, case
        assert w[0] == ic.OK and w[1] == len(case.expect), case
    lay.check(expected)
    lay.refill()
    outs = api.inflate_device_batch([lay.stream(i) for i in range(n)], fmt, [lay.dest(i) for i in range(n)], lib=gpu_lib)
    assert [size for _, size in outs] == [len(e) for e in expected]
    lay.check(expected)
    # ---- singly
    lay.refill()
    for i, case in enumerate(cases):
        r = gpu_ctx.inflate_device([lay.stream(i)], fmt, [lay.dest(i)])[0]
        assert _fields(r) == want[i], case
    lay.check(expected)


def test_size_only_mode_writes_nothing(gpu_lib, gpu_ctx):
    cases = [c for c in ic.planted_cases() if c.fmt == ic.ZLIB] + [c for c in ic.zlib_cases() if c.fmt == ic.ZLIB and len(c.expect) >= 65535]
    lay = Layout([c.stream for c in cases], [len(c.expect) for c in cases])
    n = len(cases)
    sizes = api.inflate_size_device([lay.stream(i) for i in range(n)], "zlib", lib=gpu_lib)
    assert sizes == [len(c.expect) for c in cases]
    results = gpu_ctx.inflate_device([lay.stream(i) for i in range(n)], "zlib", [None] * n)
    assert [(int(r.status), int(r.outsize)) for r in results] == [(ic.OK, len(c.expect)) for c in cases]
    lay.check([b""] * n)
    # a mixed call: every other stream stored
    outs = [lay.dest(i) if i % 2 else None for i in range(n)]
    results = gpu_ctx.inflate_device([lay.stream(i) for i in range(n)], "zlib", outs)
    assert all(r.status == ic.OK for r in results)
    lay.check([c.expect if i % 2 else b"" for i, c in enumerate(cases)])


def test_capacity_one_byte_short(gpu_lib, gpu_ctx, cpu_program):
    cases = [c for c in ic.valid_cases() if c.fmt == ic.GZIP and len(c.expect) > 0]
    caps = [len(c.expect) - 1 for c in cases]
    lay = Layout([c.stream for c in cases], caps)
    n = len(cases)
    want = cpu_program(ic.GZIP, [c.stream for c in cases], caps)
    results = gpu_ctx.inflate_device([lay.stream(i) for i in range(n)], "gzip", [lay.dest(i) for i in range(n)])
    for case, r, w in zip(cases, results, want):
        assert _fields(r) == w and r.status == ic.CAPACITY and r.outsize == len(case.expect), case
    assert gpu_lib.zmx_last_error_class() == ZMX_ERR_REFUSED
    assert f"stream 0: ZMX_INFLATE_CAPACITY (14)" in gpu_ctx.error() and f"takes {len(cases[0].expect)} bytes" in gpu_ctx.error()
    lay.check([c.expect[:-1] for c in cases])      # the byte at `capacity` and beyond: the canary's
    # Python: CapacityError with what it takes
    big = max(range(n), key=lambda i: caps[i])
    with pytest.raises(api.CapacityError) as e:
        api.inflate_device(lay.stream(big), "gzip", out=lay.dest(big), lib=gpu_lib)
    assert e.value.needed == caps[big] + 1
    with pytest.raises(api.CapacityError) as e:
        api.inflate_device_batch([lay.stream(0), lay.stream(big)], "gzip", [lay.dest(0), lay.dest(big)], lib=gpu_lib)
    assert e.value.needed == [caps[0] + 1, caps[big] + 1]
    short = torch.full((10,), FILL, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(api.CapacityError):
        api.inflate_device(lay.stream(big), "gzip", out=short[:0], lib=gpu_lib)
    assert bool((short == FILL).all())


@pytest.mark.parametrize("fmt,cases", _by_format(ic.malformed_cases() + ic.trailer_cases()), ids=["gzip", "zlib", "deflate"])
def test_malformed_streams_beside_valid_ones(gpu_lib, gpu_ctx, cpu_program, fmt, cases):
    """Every malformed stream with its status, -1, the first index in zmx_last_error(), and the valid streams of the same batch
    decoded regardless; singly through the pooled entry as well."""
    good = [c for c in ic.planted_cases() if c.fmt == fmt][:3]
    mixed = [good[0]] + cases[:len(cases) // 2] + [good[1]] + cases[len(cases) // 2:] + [good[2]]
    streams = [c.stream for c in mixed]
    caps = [len(c.expect) if c.expect is not None else 4096 for c in mixed]
    lay = Layout(streams, caps)
    n = len(mixed)
    want = cpu_program(fmt, streams, caps)
    results = gpu_ctx.inflate_device([lay.stream(i) for i in range(n)], fmt, [lay.dest(i) for i in range(n)])
    refs = [ic.inflate_ref(fmt, c.stream) for c in mixed]
    for case, r, w, ref in zip(mixed, results, want, refs):
        assert _fields(r) == w, case
        assert r.status == ref["kernel_status"], case
    lay.check([ref["out"] for ref in refs])
    lay.refill()
    with pytest.raises(api.InflateError) as e:
        api.inflate_device_batch([lay.stream(i) for i in range(n)], fmt, [lay.dest(i) for i in range(n)], lib=gpu_lib)
    assert gpu_lib.zmx_last_error_class() == ZMX_ERR_DATA
    err = e.value
    assert err.index == 1 and err.status == mixed[1].status and err.block == refs[1]["block"] and err.needed == refs[1]["outsize"]
    assert f"stream 1: ZMX_INFLATE_{ic.STATUS_NAMES[mixed[1].status]} ({mixed[1].status})" in str(err)
    assert [int(r.status) for r in err.results] == [c.status for c in mixed]     # CHECKSUM and SIZE among them
    lay.check([ref["out"] for ref in refs])
    for i, case in enumerate(mixed):
        if case.status == ic.OK:
            continue
        with pytest.raises(api.InflateError) as e:
            api.inflate_device(lay.stream(i), fmt, out=lay.dest(i), lib=gpu_lib)
        assert (e.value.index, e.value.status) == (0, case.status), case
        size = ctypes.c_size_t(0)
        fn = gpu_lib.zmx_inflate_device
        fn.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
        assert fn(fmt, *lay.stream(i), *lay.dest(i), ctypes.byref(size)) == -1 and size.value == refs[i]["outsize"], case


def _class(cls, n):
    d = torch.from_numpy(np.frombuffer(generate(cls, n), dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return d


@pytest.mark.parametrize("cls", ["T", "Z"])
def test_round_trip_of_compress_device_out(gpu_lib, cls):
    n = 1000000
    d_in = _class(cls, n)
    for fmt in (api.FORMAT_GZIP, api.FORMAT_ZLIB, api.FORMAT_DEFLATE):
        for blocksplitting in (0, 1):
            d_stream = torch.empty(api.compress_bound(n, fmt, lib=gpu_lib), dtype=torch.uint8, device="cuda:0")
            size = api.compress_device_out(d_in, d_stream, fmt, ZopfliOptions(2, blocksplitting), lib=gpu_lib)
            back = api.inflate_device(d_stream[:size], fmt, lib=gpu_lib)
            assert back.numel() == n and torch.equal(back, d_in), (cls, fmt, blocksplitting)


@pytest.mark.parametrize("align", [1, 4096])
def test_round_trip_out_of_a_packed_arena(gpu_lib, align):
    rng = np.random.default_rng(7)
    sizes = [0, 1, 65536] + [int(v) for v in rng.integers(0, 65537, size=61)]
    whole = _class("T", sum(sizes))
    srcs, at = [], 0
    for s in sizes:
        srcs.append(whole[at:at + s])
        at += s
    arena = torch.empty(api.compress_batch_bound(sizes, api.FORMAT_ZLIB, align, lib=gpu_lib), dtype=torch.uint8, device="cuda:0")
    offsets, stream_sizes = api.compress_device_batch_packed(srcs, arena, align, api.FORMAT_ZLIB, ZopfliOptions(2), lib=gpu_lib)
    assert all(o % align == 0 for o in offsets)
    backs = api.inflate_device_batch([(arena.data_ptr() + o, s) for o, s in zip(offsets, stream_sizes)], "zlib", lib=gpu_lib)
    for src, back in zip(srcs, backs):
        assert back.numel() == src.numel() and torch.equal(back, src)


def test_round_trip_of_a_png_idat(gpu_lib, gpu_ctx):
    w = h = 64
    rng = np.random.default_rng(3)
    y, x = np.mgrid[0:h, 0:w * 4]
    img = ((x // 4 * 3 + y * 2 + rng.integers(-3, 4, size=(h, w * 4))) & 255).astype(np.uint8)
    d_img = torch.from_numpy(img).cuda()
    d_file = torch.empty(api.png_bound(w, h, 6, 8, lib=gpu_lib), dtype=torch.uint8, device="cuda:0")
    size = api.png_encode_device_out((d_img.data_ptr(), w, h, 6, 8), d_file, "e", ZopfliOptions(2), lib=gpu_lib)
    head = d_file[:64].cpu().numpy().tobytes()
    assert head[:8] == b"\x89PNG\r\n\x1a\n" and head[37:41] == b"IDAT"
    idat = struct.unpack(">I", head[33:37])[0]
    assert 41 + idat + 4 + 12 == size
    scan = api.inflate_device((d_file.data_ptr() + 41, idat), "zlib", lib=gpu_lib)
    d_types = torch.empty(h, dtype=torch.uint8, device="cuda:0")
    d_rows = torch.empty(h * (4 * w + 1), dtype=torch.uint8, device="cuda:0")
    gpu_ctx.png_filter_types_device(d_img, 4 * w, h, 4, "e", d_types)
    gpu_ctx.png_filter_rows_device(d_img, 4 * w, h, 4, d_types, d_rows)
    assert torch.equal(scan, d_rows)


def test_four_megabytes_of_text(gpu_lib):
    n = 4000000
    d_in = _class("T", n)
    d_stream = torch.empty(api.compress_bound(n, lib=gpu_lib), dtype=torch.uint8, device="cuda:0")
    size = api.compress_device_out(d_in, d_stream, api.FORMAT_GZIP, ZopfliOptions(1, 0), lib=gpu_lib)
    back = api.inflate_device(d_stream[:size], "gzip", size=n, lib=gpu_lib)
    assert torch.equal(back, d_in)


def test_refusals(gpu_lib, gpu_ctx):
    data = ic.text(1000)
    stream = zlib.compress(data)
    d_stream = torch.from_numpy(np.frombuffer(stream, dtype=np.uint8).copy()).cuda()
    d_out = torch.full((2000,), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    host = np.frombuffer(stream, dtype=np.uint8).copy()

    def refused(text, streams, outs, fmt="zlib"):
        for call in (lambda: api.inflate_device_batch(streams, fmt, outs, lib=gpu_lib), lambda: gpu_ctx.inflate_device(streams, fmt, outs)):
            with pytest.raises(RuntimeError) as e:
                call()
            assert not isinstance(e.value, (api.InflateError, api.CapacityError))
            assert text in str(e.value), str(e.value)
            assert gpu_lib.zmx_last_error_class() == ZMX_ERR_REFUSED
    refused("not device memory", [(host.ctypes.data, len(stream))], [d_out])
    refused("not device memory", [d_stream], [(host.ctypes.data, len(stream))])
    refused("leaves its allocation", [(d_stream.data_ptr(), 1 << 40)], [d_out])
    refused("leaves its allocation", [d_stream], [(d_out.data_ptr(), 1 << 40)])
    both = torch.zeros(4000, dtype=torch.uint8, device="cuda:0")
    both[:len(stream)] = d_stream
    torch.cuda.synchronize()
    refused("destination 1 overlaps input 0", [both[:len(stream)], d_stream], [d_out[:1000], both[len(stream) - 1:]])
    refused("destination 1 overlaps destination 0", [d_stream, d_stream], [d_out[:1500], d_out[1499:]])
    refused("invalid ZopfliFormat 7", [d_stream], [d_out], fmt=7)
    assert bool((d_out == FILL).all()), "a refused call wrote"
    # n = 0 returns at once
    assert api.inflate_device_batch([], "gzip", [], lib=gpu_lib) == [] and gpu_ctx.inflate_device([], "gzip", []) == []
    assert api.inflate_size_device([], "deflate", lib=gpu_lib) == []
    # ... and the call that all these refusals were of goes through
    back = api.inflate_device(d_stream, "zlib", out=d_out, lib=gpu_lib)
    assert back.cpu().numpy().tobytes() == data
