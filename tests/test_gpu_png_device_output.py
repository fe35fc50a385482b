"""The PNG entries with the file left in device memory: zmx_png_encode_device_to_device, zmx_png_optimize_device_to_device,
zmx_png_encode_device_batch_packed, zmx_png_bound and zmx_png_batch_bound.  Every file is held against the one the
host-output entry gives for the same arguments — and, for the constant filter types, against a file put together without
any PNG entry — inside a destination guarded by 0xA5 on both sides, at destination offsets 0, 1 and 3.  numiterations 2."""
import os
import subprocess

import numpy as np
import pytest
import torch

import png_color_cases as cc
import png_encode_cases as ec
import png_lossy_cases as lc
from png_rows_cases import filter_rows
from zopfli_amd import ZopfliOptions, api
from zopfli_amd._build import PNG_REF

pytestmark = pytest.mark.gpu

ZMX_ERR_REFUSED = 3
ITERATIONS = 2
STRATEGIES = list(range(8)) + [ec.PREDEFINED]
GUARD = 64
FILL = 0xa5


def _opts(**kw):
    return ZopfliOptions(ITERATIONS, **kw)


class Dest:
    """`capacity` bytes of device memory `offset` bytes behind a 256-byte boundary, 0xA5 all over, guards on both sides."""

    def __init__(self, capacity, offset=0):
        self.capacity, self.at = capacity, GUARD + offset
        self.buf = torch.full((GUARD + offset + capacity + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        assert self.buf.data_ptr() % 256 == 0

    @property
    def pair(self):
        return (self.buf.data_ptr() + self.at, self.capacity)

    def file(self, size):
        """The file's bytes, after checking that nothing outside them was written."""
        host = self.buf.cpu().numpy()
        assert (host[:self.at] == FILL).all() and (host[self.at + size:] == FILL).all(), "a byte outside the file was written"
        return host[self.at:self.at + size].tobytes()

    def untouched(self):
        return bool((self.buf.cpu().numpy() == FILL).all())


def _image(shape, d_img):
    return (d_img.data_ptr(),) + tuple(shape)


def _predefined(shape, strategy):
    return ec.mixed_types(shape[1]) if strategy == ec.PREDEFINED else None


def _upload(img):
    d = torch.from_numpy(np.array(img, dtype=np.uint8, order="C")).cuda()
    torch.cuda.synchronize()
    return d


def _no_traffic(lib):
    assert api.last_input_traffic(lib)[0] == 0, "pixels went host to device"
    assert api.last_output_traffic(lib)[0] == 0, "the stream came down"


def _reference(tmp_path, shape, img, strategy):
    """The all-reference zopflipng's file, or None where it was not built."""
    if not os.path.exists(PNG_REF):
        return None
    src, dst = str(tmp_path / "in.png"), str(tmp_path / "ref.png")
    letter = "p" if strategy == ec.PREDEFINED else ec.STRATEGY_LETTERS[strategy]
    # (the input carries the types that --filters=p takes over)
    with open(src, "wb") as f:
        f.write(ec.plain_png(shape, filter_rows(img, ec.bytewidth(shape), ec.mixed_types(shape[1]))))
    r = subprocess.run([PNG_REF, "-y", "--always_zopflify", "--keepcolortype", f"--iterations={ITERATIONS}", f"--filters={letter}",
                        src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-1000:])
    with open(dst, "rb") as f:
        return f.read()


@pytest.mark.parametrize("shape", ec.SHAPES + [ec.WIDE], ids=ec.shape_id)
def test_encode_equals_the_host_output_file(gpu_lib, shape):
    lib = gpu_lib
    img = ec.pixels(shape)
    d_img = _upload(img)
    bound = api.png_bound(*shape, lib=lib)
    for strategy in STRATEGIES + ["auto"]:
        types = _predefined(shape, strategy)
        want = api.png_encode_device(_image(shape, d_img), strategy, _opts(), predefined=types, lib=lib)
        assert bound >= len(want), (shape, strategy)
        if strategy in range(5):
            # an expectation made without any PNG entry
            scan = filter_rows(img, ec.bytewidth(shape), np.full(shape[1], strategy, dtype=np.uint8))
            assert want == ec.assemble(shape, api.compress(scan.tobytes(), api.FORMAT_ZLIB, _opts(), lib=lib)), (shape, strategy)
        for offset in (0, 1, 3):
            dst = Dest(bound, offset)
            size = api.png_encode_device_out(_image(shape, d_img), dst.pair, strategy, _opts(), predefined=types, lib=lib)
            _no_traffic(lib)
            assert size == len(want) and dst.file(size) == want, (shape, strategy, offset)
    assert np.array_equal(d_img.cpu().numpy(), img), "the image changed"


@pytest.mark.parametrize("shape", [ec.SHAPES[0], ec.SHAPES[1], ec.SHAPES[6], ec.SHAPES[7]], ids=ec.shape_id)
def test_encode_equals_zopflipng(gpu_lib, tmp_path, shape):
    """One shape per colour type against the all-reference zopflipng's file, where it was built; else against the
    host-output entry's."""
    img = ec.pixels(shape)
    d_img = _upload(img)
    for strategy in (6, 7, ec.PREDEFINED):
        dst = Dest(api.png_bound(*shape, lib=gpu_lib), 1)
        size = api.png_encode_device_out(_image(shape, d_img), dst.pair, strategy, _opts(), predefined=_predefined(shape, strategy), lib=gpu_lib)
        ref = _reference(tmp_path, shape, img, strategy)
        if ref is None:
            ref = api.png_encode_device(_image(shape, d_img), strategy, _opts(), predefined=_predefined(shape, strategy), lib=gpu_lib)
        assert dst.file(size) == ref, (shape, strategy)


def _noise(w, h):
    return np.random.default_rng(w + h).integers(0, 256, size=(h, w * 4), dtype=np.uint8)


def _gradient(w, h):
    rng = np.random.default_rng(w * 7 + h)
    y, x = np.mgrid[0:h, 0:w * 4]
    return ((x // 4 * 3 + y * 2 + rng.integers(-3, 4, size=(h, w * 4))) & 255).astype(np.uint8)


def test_noise_stored_blocks_and_two_crc_pieces(gpu_lib):
    """300 x 300 RGBA8 noise: the stored blocks' bytes come from the call's own scanline buffer, the stream is above 256 KiB
    — two CRC pieces — and the IDAT begins at file offset 37, so every destination offset is another absolute alignment.
    Capacity: exactly the size does, a byte less raises CapacityError with the size and writes nothing."""
    lib = gpu_lib
    shape = (300, 300, 6, 8)
    d_img = _upload(_noise(300, 300))
    want = api.png_encode_device(_image(shape, d_img), 0, _opts(), lib=lib)
    size = len(want)
    assert size > 262144 + 57 and api.png_bound(*shape, lib=lib) >= size
    for offset in (0, 1, 2, 3):
        dst = Dest(size, offset)   # exactly the size
        assert api.png_encode_device_out(_image(shape, d_img), dst.pair, 0, _opts(), lib=lib) == size
        _no_traffic(lib)
        assert dst.file(size) == want, offset
    short = Dest(size - 1, 1)
    with pytest.raises(api.CapacityError) as e:
        api.png_encode_device_out(_image(shape, d_img), short.pair, 0, _opts(), lib=lib)
    assert e.value.needed == size and short.untouched()


@pytest.mark.parametrize("blocksplitting", [0, 1])
def test_two_master_blocks(gpu_lib, blocksplitting):
    """600 x 600 RGBA8, a gradient with noise: 1 440 600 bytes of scanlines, two master blocks."""
    lib = gpu_lib
    shape = (600, 600, 6, 8)
    d_img = _upload(_gradient(600, 600))
    opts = _opts(blocksplitting=blocksplitting)
    want = api.png_encode_device(_image(shape, d_img), 1, opts, lib=lib)
    bound = api.png_bound(*shape, lib=lib)
    assert bound >= len(want)
    dst = Dest(bound, 3)
    size = api.png_encode_device_out(_image(shape, d_img), dst.pair, 1, opts, lib=lib)
    _no_traffic(lib)
    assert size == len(want) and dst.file(size) == want


def test_smallest_file(gpu_lib):
    """1 x 1 grey."""
    lib = gpu_lib
    shape = (1, 1, 0, 8)
    d_img = _upload(np.array([[77]], dtype=np.uint8))
    want = api.png_encode_device(_image(shape, d_img), "e", _opts(), lib=lib)
    size = len(want)
    assert api.png_bound(*shape, lib=lib) >= size
    for offset in (0, 1, 3):
        dst = Dest(size, offset)
        assert api.png_encode_device_out(_image(shape, d_img), dst.pair, "e", _opts(), lib=lib) == size
        assert dst.file(size) == want
    short = Dest(size - 1)
    with pytest.raises(api.CapacityError) as e:
        api.png_encode_device_out(_image(shape, d_img), short.pair, "e", _opts(), lib=lib)
    assert e.value.needed == size and short.untouched()


def _color_case(prefix):
    return next(c for c in cc.CASES if c[0].startswith(prefix))


# palette, key, 1-bit grey, RGBA -> RGB, 16 -> 8, and two palette icons below 4096 bytes: the second try replaces the first, and does not
OPTIMIZE_CASES = ["colors-5", "key", "grey1-w37-ct", "colors-257", "fake16", "colors-1", "retry-100-alpha"]


@pytest.mark.parametrize("name", OPTIMIZE_CASES)
def test_optimize_equals_the_host_output_file(gpu_lib, name):
    lib = gpu_lib
    case = _color_case(name)
    shape = case[1:]
    d_img = _upload(cc.pixels(case))
    bound = api.png_bound(*shape, lib=lib)
    for strategy in (0, 6, "auto"):
        want = api.png_optimize_device(_image(shape, d_img), strategy, _opts(), lib=lib)
        assert bound >= len(want), (name, strategy)
        for offset in (0, 3):
            dst = Dest(bound, offset)
            size = api.png_optimize_device_out(_image(shape, d_img), dst.pair, strategy, _opts(), lib=lib)
            _no_traffic(lib)
            assert size == len(want) and dst.file(size) == want, (name, strategy, offset)
    # capacity is held against the file that is kept
    exact = Dest(len(want), 1)
    assert api.png_optimize_device_out(_image(shape, d_img), exact.pair, "auto", _opts(), lib=lib) == len(want)
    assert exact.file(len(want)) == want
    short = Dest(len(want) - 1, 1)
    with pytest.raises(api.CapacityError) as e:
        api.png_optimize_device_out(_image(shape, d_img), short.pair, "auto", _opts(), lib=lib)
    assert e.value.needed == len(want) and short.untouched()
    assert np.array_equal(d_img.cpu().numpy(), cc.pixels(case)), "the image changed"


@pytest.mark.parametrize("name,flags", [("retry-wins", dict(lossy_transparent=True)), ("rgba16-hi", dict(lossy_8bit=True)),
                                        ("rgba16-hi", dict(lossy_transparent=True, lossy_8bit=True))])
def test_lossy_flags(gpu_lib, name, flags):
    lib = gpu_lib
    case = lc.case(name)
    shape = case[1:]
    d_img = _upload(lc.pixels(case))
    for optimize in (True, False):
        host_fn, dev_fn = (api.png_optimize_device, api.png_optimize_device_out) if optimize else (api.png_encode_device, api.png_encode_device_out)
        want = host_fn(_image(shape, d_img), 2, _opts(), lib=lib, **flags)
        dst = Dest(api.png_bound(*shape, lib=lib), 1)
        size = dev_fn(_image(shape, d_img), dst.pair, 2, _opts(), lib=lib, **flags)
        _no_traffic(lib)
        assert size == len(want) and dst.file(size) == want, (name, flags, optimize)
    assert np.array_equal(d_img.cpu().numpy(), lc.pixels(case)), "the caller's image changed"


def _packed_offsets(sizes, align):
    out, end = [], 0
    for s in sizes:
        out.append((end + align - 1) // align * align)
        end = out[-1] + s
    return out, end


def test_batch_packed(gpu_lib):
    lib = gpu_lib
    shapes = ec.SHAPES + [ec.WIDE]
    imgs = [_upload(ec.pixels(s)) for s in shapes]
    images = [_image(s, d) for s, d in zip(shapes, imgs)]
    singles = [api.png_encode_device(im, 6, _opts(), lib=lib) for im in images]
    orders = [list(range(11)), [7, 3, 10, 0, 9, 1, 8, 2, 6, 4, 5]]
    for order, align in ((orders[0], 1), (orders[1], 16), (orders[0], 4096), ([4], 16)):
        batch = [images[i] for i in order]
        want = [singles[i] for i in order]
        bound = api.png_batch_bound(batch, align, lib=lib)
        offs, end = _packed_offsets([len(w) for w in want], align)
        assert bound >= end
        arena = Dest(bound, 0)
        got_offs, got_sizes = api.png_encode_device_batch_packed(batch, arena.pair, align, 6, _opts(), lib=lib)
        _no_traffic(lib)
        assert got_sizes == [len(w) for w in want] and got_offs == offs, (order, align)
        host = arena.buf.cpu().numpy()
        written = np.zeros(host.size, dtype=bool)
        for off, w in zip(offs, want):
            assert host[arena.at + off:arena.at + off + len(w)].tobytes() == w, (order, align, off)
            written[arena.at + off:arena.at + off + len(w)] = True
        assert (host[~written] == FILL).all(), "a byte between the files or behind the last was written"
        # an arena one byte short: the same offsets and sizes, nothing written
        short = Dest(end - 1, 0)
        with pytest.raises(api.CapacityError) as e:
            api.png_encode_device_batch_packed(batch, short.pair, align, 6, _opts(), lib=lib)
        assert e.value.needed == [len(w) for w in want] and short.untouched()
    assert api.png_encode_device_batch_packed([], Dest(16).pair, 1, 6, _opts(), lib=lib) == ([], [])
    assert api.png_batch_bound([], 1, lib=lib) == 0
    # lossy flags and the automatic choice go through the batch as through the single call
    auto = [api.png_encode_device(im, "auto", _opts(), lib=lib, lossy_transparent=True) for im in images[:4]]
    arena = Dest(api.png_batch_bound(images[:4], 1, lib=lib))
    offs, sizes = api.png_encode_device_batch_packed(images[:4], arena.pair, 1, "auto", _opts(), lib=lib, lossy_transparent=True)
    host = arena.buf.cpu().numpy()
    assert [host[arena.at + o:arena.at + o + s].tobytes() for o, s in zip(offs, sizes)] == auto
    with pytest.raises(RuntimeError) as e:
        api.png_encode_device_batch_packed(images[:2], Dest(1 << 16).pair, 1, "p", _opts(), lib=lib)
    assert lib.zmx_last_error_class() == ZMX_ERR_REFUSED and not isinstance(e.value, api.CapacityError)
    for align in (0, 3, 8192):
        with pytest.raises(RuntimeError):
            api.png_encode_device_batch_packed(images[:2], Dest(1 << 16).pair, align, 6, _opts(), lib=lib)
        assert lib.zmx_last_error_class() == ZMX_ERR_REFUSED


def test_refusals_write_nothing(gpu_lib):
    """d_out in host memory, overlapping the image, leaving its allocation: ZMX_ERR_REFUSED before anything runs."""
    lib = gpu_lib
    shape = (16, 16, 6, 8)
    pixels = np.random.default_rng(3).integers(0, 256, size=(16, 64), dtype=np.uint8)
    room = torch.full((1 << 16,), FILL, dtype=torch.uint8, device="cuda:0")
    room[:1024] = torch.from_numpy(pixels.reshape(-1)).cuda()
    torch.cuda.synchronize()
    before = room.cpu().numpy().copy()
    image = (room.data_ptr(), 16, 16, 6, 8)
    on_host = np.full(1 << 16, FILL, dtype=np.uint8)
    refused = [
        ("host memory", (on_host.ctypes.data, 1 << 16)),
        ("overlaps the image", (room.data_ptr() + 1000, 4096)),
        ("overlaps the image from below", (room.data_ptr(), 4096)),
        ("leaves its allocation", (room.data_ptr() + 2048, 1 << 40)),
        ("null with a capacity", (0, 4096)),
    ]
    for what, dst in refused:
        for fn in (api.png_encode_device_out, api.png_optimize_device_out):
            with pytest.raises(RuntimeError) as e:
                fn(image, dst, 6, _opts(), lib=lib)
            assert lib.zmx_last_error_class() == ZMX_ERR_REFUSED and not isinstance(e.value, api.CapacityError), (what, str(e.value))
        with pytest.raises(RuntimeError):
            api.png_encode_device_batch_packed([image, image], dst, 1, 6, _opts(), lib=lib)
        assert lib.zmx_last_error_class() == ZMX_ERR_REFUSED, what
    assert np.array_equal(room.cpu().numpy(), before) and (on_host == FILL).all(), "a refused call wrote something"
    # what the host-output entries refuse of the image and the strategy, with a good destination
    good = (room.data_ptr() + 4096, 8192)
    for what, im, strategy, types in [("width 0", (room.data_ptr(), 0, 16, 6, 8), 6, None), ("palette input", (room.data_ptr(), 16, 16, 3, 8), 6, None),
                                      ("strategy 9", image, 9, None), ("predefined without types", image, 8, None),
                                      ("null pixels", (0, 16, 16, 6, 8), 6, None)]:
        with pytest.raises(RuntimeError):
            api.png_encode_device_out(im, good, strategy, _opts(), predefined=types, lib=lib)
        assert lib.zmx_last_error_class() == ZMX_ERR_REFUSED, what
    assert np.array_equal(room.cpu().numpy(), before)
    assert api.png_bound(16, 16, 3, 8, lib=lib) == 0 and api.png_bound(0, 16, 6, 8, lib=lib) == 0
    # and the next valid call is right
    size = api.png_encode_device_out(image, good, 6, _opts(), lib=lib)
    assert room[4096:4096 + size].cpu().numpy().tobytes() == api.png_encode_device(image, 6, _opts(), lib=lib)
