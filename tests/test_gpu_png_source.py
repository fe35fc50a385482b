"""Strided, planar, float and 16-bit sources in device memory: k_png_pack and the zmx_png_*_source_* entries on the cases
of tests/png_source_cases.py.  Context.png_pack_device is held byte for byte against the numpy model for every case at
every destination alignment, by a launch of its own and as one batch launch, guard bytes and sources untouched.  Every
_source entry is held to the existing entry of the packed image — the model's bytes, uploaded —: the files must be equal.
The bounds, a capacity one byte short, the refusals that need a device, and the existing Python entries with today's
arguments.  numiterations 2; nothing is larger than 256 x 256."""
import ctypes

import numpy as np
import pytest
import torch

import png_source_cases as sc
from zopfli_amd import Context, ZopfliOptions, api

pytestmark = pytest.mark.gpu

ZMX_ERR_REFUSED = 3
ITERATIONS = 2
GUARD = 64
FILL = 0xa5
STRATEGIES = ["e", "0", "4", "b", "auto", "p"]
LOSSY = [{}, {"lossy_transparent": True}, {"lossy_8bit": True}]
ENTRY_NAMES = ["combo-f32-8-c4-CHW", "pitch-u8-8", "combo-u16-16-c3-CHW", "bgra-chw-f16-16", "bottom-up-bf16-8", "broadcast-f32-16",
               "combo-u8-8-c2-HWC", "xstep2-u16-16"]


def _opts():
    return ZopfliOptions(ITERATIONS)


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    c = Context(0, gpu_lib)
    yield c
    c.close()


@pytest.fixture(scope="module")
def want():
    return {c.name: sc.pack(c) for c in sc.CASES}


class Resident:
    """Every case's allocation in ONE device tensor, case k at a 16-byte boundary plus 4 * (k % 4)."""

    def __init__(self, cases):
        self.start, at = {}, 0
        for k, c in enumerate(cases):
            at = (at + 15) // 16 * 16 + 4 * (k % 4)
            self.start[c.name] = at
            at += len(c.buf)
        self.host = np.full(at + 16, 0x5a, dtype=np.uint8)
        for c in cases:
            self.host[self.start[c.name]:self.start[c.name] + len(c.buf)] = c.buf
        self.dev = torch.from_numpy(self.host.copy()).to("cuda:0")
        torch.cuda.synchronize()

    def source(self, c):
        ptr = self.dev.data_ptr() + self.start[c.name] + c.offset
        return api.PngSource((ptr, c.sy, c.sx, c.sc, c.width, c.height, c.channels, c.sample, c.depth, c.order))

    def unchanged(self):
        return np.array_equal(self.dev.cpu().numpy(), self.host)


@pytest.fixture(scope="module")
def resident():
    return Resident(sc.CASES)


def _layout(cases, mod):
    """Destinations one behind the other, each `mod` bytes behind a 16-byte boundary with GUARD bytes in front."""
    at, where = 0, []
    for c in cases:
        at = (at + GUARD + 15) // 16 * 16 + mod
        where.append(at)
        at += c.nbytes
    return where, at + GUARD


def _check_destinations(d_out, cases, where, want, what):
    host = d_out.cpu().numpy()
    mine = np.zeros(host.size, dtype=bool)
    for c, at in zip(cases, where):
        got = host[at:at + c.nbytes].tobytes()
        assert got == want[c.name], (c.name, what)
        mine[at:at + c.nbytes] = True
    assert (host[~mine] == FILL).all(), (what, "a byte outside the packed images was written")


@pytest.mark.parametrize("mod", range(16))
def test_pack_every_case(ctx, resident, want, mod):
    """Every case at destination alignment `mod`: a launch of its own each, then all of them as one launch."""
    cases = sc.CASES
    where, size = _layout(cases, mod)
    sources = [resident.source(c) for c in cases]
    d_out = torch.full((size,), FILL, dtype=torch.uint8, device="cuda:0")
    assert d_out.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    base = d_out.data_ptr()
    for c, s, at in zip(cases, sources, where):
        ctx.png_pack_device([s], [(base + at, c.nbytes)])
    _check_destinations(d_out, cases, where, want, "single")
    d_out.fill_(FILL)
    torch.cuda.synchronize()
    ctx.png_pack_device(sources, [(base + at, c.nbytes) for c, at in zip(cases, where)])
    _check_destinations(d_out, cases, where, want, "batch")
    assert resident.unchanged(), "a source changed"


def test_pack_neighbours_share_vectors(ctx, resident, want):
    """The batch on the binary search's edges with no byte between its destinations: one byte between two large images."""
    cases = sc.BATCH_EDGE + [sc.case("combo-f16-16-c3-CHW"), sc.case("shape-1x1x1-HWC-u8-8")] + sc.BATCH_EDGE[3:4]
    for first in (GUARD, GUARD + 5):
        where, at = [], first
        for c in cases:
            where.append(at)
            at += c.nbytes
        d_out = torch.full((at + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        ctx.png_pack_device([resident.source(c) for c in cases], [(d_out.data_ptr() + w, c.nbytes) for c, w in zip(cases, where)])
        _check_destinations(d_out, cases, where, want, f"adjacent from {first}")


def test_pack_nothing(ctx):
    ctx.png_pack_device([], [])


def test_pack_tensors(ctx, gpu_lib):
    """PngSource of torch tensors as they lie: CHW float, a crop of a BGRA frame, a [::2] view, an expand()."""
    g = torch.Generator(device="cpu").manual_seed(7)
    chw = (torch.rand(4, 33, 47, generator=g) * 1.2 - 0.1).to("cuda:0")
    frame = torch.randint(0, 256, (40, 64, 4), generator=g, dtype=torch.uint8).to("cuda:0")
    half = torch.rand(3, 20, 30, generator=g).to(torch.float16).to("cuda:0")
    bf = torch.rand(21, 19, generator=g).to(torch.bfloat16).to("cuda:0")
    u16 = torch.from_numpy(np.random.default_rng(3).integers(0, 65536, size=(3, 9, 14), dtype=np.uint16)).to("cuda:0")
    tries = [
        (api.PngSource(chw, "CHW"), (chw.cpu() * 255 + 0.5).clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous().numpy().tobytes()),
        (api.PngSource(frame[:37, :51], "HWC", "BGRA"),
         frame[:37, :51].cpu()[:, :, [2, 1, 0, 3]].contiguous().numpy().tobytes()),
        (api.PngSource(half[:, ::2, ::2], "CHW", (1, 2, 0), bitdepth=16),
         (half[:, ::2, ::2].cpu().float() * 65535 + 0.5).clamp(0, 65535).to(torch.int32)[[1, 2, 0]].permute(1, 2, 0).contiguous().numpy().astype(">u2").tobytes()),
        (api.PngSource(bf.unsqueeze(0).expand(3, -1, -1), "CHW"),
         (bf.cpu().float() * 255 + 0.5).clamp(0, 255).to(torch.uint8).unsqueeze(2).expand(-1, -1, 3).contiguous().numpy().tobytes()),
        (api.PngSource(u16, "CHW"), u16.cpu().numpy().transpose(1, 2, 0).astype(">u2").tobytes()),
    ]
    outs = [torch.full((len(w) + 3,), FILL, dtype=torch.uint8, device="cuda:0") for _, w in tries]
    ctx.png_pack_device([s for s, _ in tries], [(o.data_ptr() + 3, len(w)) for o, (_, w) in zip(outs, tries)])
    for k, (o, (s, w)) in enumerate(zip(outs, tries)):
        assert o.cpu().numpy()[3:].tobytes() == w, k
        assert api.png_source_image(s, gpu_lib)[4] == len(w)


# ---- the entries
def _packed_image(c, want):
    """The packed image as the existing entries take it: (the tensor that owns it, the tuple)."""
    d = torch.from_numpy(np.frombuffer(want[c.name], dtype=np.uint8).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return d, (d.data_ptr(),) + c.mode


def _types(c):
    return [(3 * r + c.width) % 5 for r in range(c.height)]


@pytest.mark.parametrize("name", ENTRY_NAMES)
def test_host_output_entries(gpu_lib, resident, want, name):
    c = sc.case(name)
    keep, image = _packed_image(c, want)
    src = resident.source(c)
    for strategy in STRATEGIES:
        predefined = _types(c) if strategy == "p" else None
        for lossy in LOSSY:
            for fn in (api.png_encode_device, api.png_optimize_device):
                got = fn(src, strategy, _opts(), predefined, gpu_lib, **lossy)
                assert api.last_input_traffic(gpu_lib)[0] == 0, "pixels went host to device"
                assert got == fn(image, strategy, _opts(), predefined, gpu_lib, **lossy), (name, strategy, lossy, fn.__name__)
                assert got[:8] == b"\x89PNG\r\n\x1a\n"
    assert resident.unchanged()


@pytest.mark.parametrize("name", ENTRY_NAMES[:4])
def test_to_device_entries(gpu_lib, resident, want, name):
    """The file left in device memory at an odd address: the host-output file of the packed image."""
    c = sc.case(name)
    keep, image = _packed_image(c, want)
    src = resident.source(c)
    bound = api.png_bound(src, lib=gpu_lib)
    assert bound == api.png_bound(*c.mode, lib=gpu_lib) > 0
    for strategy in STRATEGIES:
        predefined = _types(c) if strategy == "p" else None
        for lossy in LOSSY:
            for fn, host in ((api.png_encode_device_out, api.png_encode_device), (api.png_optimize_device_out, api.png_optimize_device)):
                d_out = torch.full((GUARD + 7 + bound + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
                torch.cuda.synchronize()
                size = fn(src, (d_out.data_ptr() + GUARD + 7, bound), strategy, _opts(), predefined, gpu_lib, **lossy)
                assert api.last_input_traffic(gpu_lib)[0] == 0
                h = d_out.cpu().numpy()
                assert h[GUARD + 7:GUARD + 7 + size].tobytes() == host(image, strategy, _opts(), predefined, gpu_lib, **lossy), (name, strategy, lossy)
                assert (h[:GUARD + 7] == FILL).all() and (h[GUARD + 7 + size:] == FILL).all()


def test_capacity_one_byte_short(gpu_lib, resident, want):
    c = sc.case("combo-f32-8-c4-CHW")
    src = resident.source(c)
    for fn, host in ((api.png_encode_device_out, api.png_encode_device), (api.png_optimize_device_out, api.png_optimize_device)):
        need = len(host(src, "e", _opts(), None, gpu_lib))
        d_out = torch.full((need + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        with pytest.raises(api.CapacityError) as e:
            fn(src, (d_out.data_ptr(), need - 1), "e", _opts(), None, gpu_lib)
        assert e.value.needed == need and (d_out.cpu().numpy() == FILL).all()
        assert fn(src, (d_out.data_ptr(), need), "e", _opts(), None, gpu_lib) == need


BATCH_NAMES = ENTRY_NAMES + ["batch-one-byte", "whole-bf16-16-c3-CHW", "shape-1x1x1-HWC-u8-8"]


@pytest.mark.parametrize("strategy", STRATEGIES[:5])
def test_batch_entries(gpu_lib, resident, want, strategy):
    cases = [sc.case(n) for n in BATCH_NAMES]
    keep = [_packed_image(c, want) for c in cases]
    images = [im for _, im in keep]
    sources = [resident.source(c) for c in cases]
    assert api.png_batch_bound(sources, 64, gpu_lib) == api.png_batch_bound(images, 64, gpu_lib) > 0
    for lossy in LOSSY:
        for fn in (api.png_encode_device_batch, api.png_optimize_device_batch):
            got = fn(sources, strategy, _opts(), gpu_lib, **lossy)
            assert api.last_input_traffic(gpu_lib)[0] == 0
            assert got == fn(images, strategy, _opts(), gpu_lib, **lossy), (strategy, lossy, fn.__name__)
        files = api.png_encode_device_batch(images, strategy, _opts(), gpu_lib, **lossy)
        for align in (1, 64):
            bound = api.png_batch_bound(sources, align, gpu_lib)
            arena = torch.full((bound + 64,), FILL, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            offsets, sizes = api.png_encode_device_batch_packed(sources, (arena.data_ptr(), bound), align, strategy, _opts(), gpu_lib, **lossy)
            assert api.last_input_traffic(gpu_lib)[0] == 0
            h = arena.cpu().numpy()
            assert (offsets, sizes) == api.png_encode_device_batch_packed(images, (arena.data_ptr(), bound), align, strategy, _opts(), gpu_lib, **lossy)
            for off, size, f in zip(offsets, sizes, files):
                assert off % align == 0 and h[off:off + size].tobytes() == f
            assert (h[bound:] == FILL).all()


def test_batch_out_of_one_nchw_tensor(gpu_lib):
    """Views out of one NCHW float32 tensor, nothing copied: the files of the torch chain's images."""
    g = torch.Generator(device="cpu").manual_seed(11)
    batch = torch.rand(6, 4, 16, 20, generator=g).to("cuda:0")
    chain = [(x.clamp(0, 1) * 255 + 0.5).to(torch.uint8).permute(1, 2, 0).contiguous() for x in batch]
    sources = api.png_sources(batch)
    assert all(s.struct.d_data == batch[i].data_ptr() for i, s in enumerate(sources))
    got = api.png_encode_device_batch(sources, "e", _opts(), gpu_lib)
    assert api.last_input_traffic(gpu_lib)[0] == 0
    assert got == api.png_encode_device_batch(chain, "e", _opts(), gpu_lib)
    nhwc = batch.permute(0, 2, 3, 1)
    assert api.png_optimize_device_batch(api.png_sources(nhwc, "NHWC"), "auto", _opts(), gpu_lib) == api.png_optimize_device_batch(chain, "auto", _opts(), gpu_lib)


def test_sixteen_bit_rgba_through_lossy_8bit(gpu_lib):
    rng = np.random.default_rng(5)
    host = rng.integers(0, 65536, size=(4, 12, 18), dtype=np.uint16)
    host[3, :4] = 0
    u16 = torch.from_numpy(host).to("cuda:0")
    packed = torch.from_numpy(np.frombuffer(host.transpose(1, 2, 0).astype(">u2").tobytes(), dtype=np.uint8).copy()).to("cuda:0")
    image = (packed.data_ptr(), 18, 12, 6, 16)
    src = api.PngSource(u16, "CHW")
    for lossy in ({"lossy_8bit": True}, {"lossy_8bit": True, "lossy_transparent": True}):
        got = api.png_optimize_device(src, "e", _opts(), None, gpu_lib, **lossy)
        assert got == api.png_optimize_device(image, "e", _opts(), None, gpu_lib, **lossy)
        assert got[24] == 8, "the file is not 8 bits deep"
    # (uint16 to an 8-bit PNG directly is refused: the flag is the way)
    with pytest.raises(RuntimeError, match="not narrowed"):
        api.png_encode_device(api.PngSource(u16, "CHW", bitdepth=8), "e", _opts(), None, gpu_lib)
    assert gpu_lib.zmx_last_error_class() == ZMX_ERR_REFUSED


# ---- refusals that need a device
def _call_single(lib, name, src, out, outsize):
    fn = getattr(lib, name)
    fn.argtypes = [ctypes.POINTER(api.ZopfliOptions), ctypes.POINTER(api.PngSourceStruct), ctypes.c_int, ctypes.c_char_p, ctypes.c_uint,
                   ctypes.POINTER(api._u8p), ctypes.POINTER(ctypes.c_size_t)]
    fn.restype = ctypes.c_int
    return fn(ctypes.byref(_opts()), ctypes.byref(src.struct), 6, None, 0, ctypes.byref(out), ctypes.byref(outsize))


def test_refusals(ctx, gpu_lib, resident, want):
    lib = gpu_lib
    good = [resident.source(sc.case(n)) for n in ("combo-u8-8-c4-HWC", "combo-f32-8-c3-CHW", "pitch-u8-8")]
    host_mem = np.zeros(4096, dtype=np.uint8)
    in_host = api.PngSource((host_mem.ctypes.data, 64, 4, 1, 16, 16, 4, 0, 8))
    own = torch.zeros(16 * 64, dtype=torch.uint8, device="cuda:0")
    try:
        # sample (0, 0, 0) and everything behind it lie in the tensor, the rows run DOWN from it, a GiB each: the first byte
        # any sample touches lies 15 GiB in front of the allocation's, and only the extent says so
        leaves = api.PngSource((own.data_ptr(), -(1 << 30), 4, 1, 16, 16, 4, 0, 8))
        dst = torch.full((3 * 4096,), FILL, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        sentinel = ctypes.cast(ctypes.c_void_p(0x1234), api._u8p)
        # (the byte 15 GiB in front is no device memory at all, or another allocation's that ends long before the tensor)
        for bad, texts in ((in_host, ("not device memory",)), (leaves, ("not device memory", "leaves its allocation", "unknown"))):
            for at in range(3):
                sources = list(good)
                sources[at] = bad
                # the pack step
                with pytest.raises(RuntimeError) as e:
                    ctx.png_pack_device(sources, [(dst.data_ptr() + 4096 * k, 4096) for k in range(3)])
                assert f"source {at}: the extent" in str(e.value) and any(t in str(e.value) for t in texts), str(e.value)
                assert lib.zmx_last_error_class() == ZMX_ERR_REFUSED
                # the batches
                for fn in (api.png_encode_device_batch, api.png_optimize_device_batch):
                    with pytest.raises(RuntimeError) as e:
                        fn(sources, "e", _opts(), lib)
                    assert f"source {at}: the extent" in str(e.value) and any(t in str(e.value) for t in texts), str(e.value)
                    assert lib.zmx_last_error_class() == ZMX_ERR_REFUSED
                with pytest.raises(RuntimeError) as e:
                    api.png_encode_device_batch_packed(sources, (dst.data_ptr(), 3 * 4096), 1, "e", _opts(), lib)
                assert f"source {at}" in str(e.value) and not isinstance(e.value, api.CapacityError)
            # the single entries: out and outsize as they were
            for name in ("zmx_png_encode_source_device", "zmx_png_optimize_source_device"):
                out, outsize = sentinel, ctypes.c_size_t(0)
                assert _call_single(lib, name, bad, out, outsize) != 0
                assert ctypes.cast(out, ctypes.c_void_p).value == 0x1234 and outsize.value == 0
                assert "source 0" in (lib.zmx_last_error() or b"").decode() and lib.zmx_last_error_class() == ZMX_ERR_REFUSED
            for fn in (api.png_encode_device_out, api.png_optimize_device_out):
                with pytest.raises(RuntimeError) as e:
                    fn(bad, (dst.data_ptr(), 3 * 4096), "e", _opts(), None, lib)
                assert "source 0" in str(e.value) and not isinstance(e.value, api.CapacityError)
        assert (dst.cpu().numpy() == FILL).all(), "a refused call wrote"
        # a destination inside a source's extent — between the rows of a pitched frame, where no sample lies
        c = sc.case("pitch-u8-8")
        src = resident.source(c)
        gap = src.struct.d_data + c.width * 4 + 1
        before = resident.dev.clone()
        for fn in (api.png_encode_device_out, api.png_optimize_device_out):
            with pytest.raises(RuntimeError) as e:
                fn(src, (gap, c.sy * (c.height - 1) - 8), "e", _opts(), None, lib)
            assert "overlaps" in str(e.value) and lib.zmx_last_error_class() == ZMX_ERR_REFUSED
        with pytest.raises(RuntimeError) as e:
            api.png_encode_device_batch_packed([good[0], src], (gap, c.sy * (c.height - 1) - 8), 1, "e", _opts(), lib)
        assert "overlaps image 1" in str(e.value)
        with pytest.raises(RuntimeError) as e:
            ctx.png_pack_device([good[0], src], [(dst.data_ptr(), 4096), (gap, c.nbytes)])
        assert "source 1" in str(e.value) and "overlaps its extent" in str(e.value)
        with pytest.raises(RuntimeError) as e:
            ctx.png_pack_device([good[0], good[0]], [(dst.data_ptr(), 4096), (dst.data_ptr() + 100, 4096)])
        assert "source 1" in str(e.value) and "overlaps" in str(e.value)
        # a capacity below the packed size, a destination in host memory
        with pytest.raises(RuntimeError, match="source 1.*capacity"):
            ctx.png_pack_device([good[0], good[0]], [(dst.data_ptr(), 4096), (dst.data_ptr() + 4096, sc.case("combo-u8-8-c4-HWC").nbytes - 1)])
        with pytest.raises(RuntimeError, match="source 0.*destination"):
            ctx.png_pack_device([good[0]], [(host_mem.ctypes.data, 4096)])
        torch.cuda.synchronize()
        assert torch.equal(before, resident.dev) and (dst.cpu().numpy() == FILL).all()
    finally:
        del own


def test_existing_entries_take_todays_arguments(gpu_lib):
    """One image through the old path and as a PngSource of the same contiguous uint8 tensor: equal files; tuples, tensors and
    bounds give what they gave."""
    g = torch.Generator(device="cpu").manual_seed(3)
    t = torch.randint(0, 256, (24, 31, 3), generator=g, dtype=torch.uint8).to("cuda:0")
    old = api.png_encode_device(t, "e", _opts(), None, gpu_lib)
    assert old == api.png_encode_device((t.data_ptr(), 31, 24, 2, 8), "e", _opts(), None, gpu_lib)
    assert old == api.png_encode_device(api.PngSource(t), "e", _opts(), None, gpu_lib)
    assert api.png_optimize_device(t, "auto", _opts(), None, gpu_lib) == api.png_optimize_device(api.PngSource(t), "auto", _opts(), None, gpu_lib)
    assert api.png_encode_device_batch([t, t[:5].contiguous()], "0", _opts(), gpu_lib)[0] == api.png_encode_device(t, "0", _opts(), None, gpu_lib)
    assert api.png_bound(31, 24, 2, 8, gpu_lib) == api.png_bound(api.PngSource(t), lib=gpu_lib)
    assert api.png_batch_bound([t, (0, 5, 5, 6, 16)], 16, gpu_lib) > 0
    with pytest.raises(ValueError):
        api.png_encode_device(t.permute(2, 0, 1), "e", _opts(), None, gpu_lib)   # (not contiguous: still today's error)
    with pytest.raises(ValueError):
        api.png_encode_device_batch([t, api.PngSource(t)], "e", _opts(), gpu_lib)
