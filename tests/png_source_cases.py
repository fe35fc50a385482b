"""Strided, planar, float and 16-bit sources of the device PNG entries (zmx_png_source, include/zopfli_amd.h): a plain
numpy model of the packed image — gather by strides, `order`, the fp32 quantisation in numpy.float32, big-endian output —
and the cases that stand on k_png_pack's edges (zopfli_amd/csrc/device/zmx_png_pack.h).  A case holds its allocation's bytes
and says where sample (0, 0, 0) lies in it; nothing here knows the kernel."""
import itertools
import struct
import zlib

import numpy as np

U8, U16, F16, BF16, F32 = 0, 1, 2, 3, 4   # ZMX_PNG_SAMPLE_*
SAMPLE_BYTES = {U8: 1, U16: 2, F16: 2, BF16: 2, F32: 4}
SAMPLE_NAMES = {U8: "u8", U16: "u16", F16: "f16", BF16: "bf16", F32: "f32"}
COLORTYPE = {1: 0, 2: 4, 3: 2, 4: 6}
# every (sample, bitdepth) the entries take
COMBOS = ((U8, 8), (U16, 16), (F16, 8), (F16, 16), (BF16, 8), (BF16, 16), (F32, 8), (F32, 16))
TILE_BYTES = 768 * 16   # kPngPackTileVecs vectors of a destination

WIDTHS = (1, 2, 3, 5, 15, 16, 17, 63, 64, 65, 257)
HEIGHTS = (1, 2, 3, 7)


class Case:
    """buf: the allocation (uint8); sample (y, x, c) lies at buf[offset + y * sy + x * sx + c * sc]."""

    def __init__(self, name, buf, offset, strides, width, height, channels, sample, depth, order):
        self.name, self.buf, self.offset = name, np.ascontiguousarray(buf, dtype=np.uint8), int(offset)
        self.sy, self.sx, self.sc = (int(s) for s in strides)
        self.width, self.height, self.channels, self.sample, self.depth = width, height, channels, sample, depth
        self.order = tuple(order) + (0,) * (4 - len(order))

    @property
    def nbytes(self):
        return self.width * self.height * self.channels * self.depth // 8

    @property
    def mode(self):
        return self.width, self.height, COLORTYPE[self.channels], self.depth

    def record(self, src_mod=0, dst_mod=0, fake=0, with_buf=True):
        """The case as tests/hostlib/png_source_print.cc reads it."""
        buf = self.buf.tobytes() if with_buf else b""
        return struct.pack("<QQqqqqIIIII4sII", len(buf), fake, self.offset, self.sy, self.sx, self.sc, self.width, self.height, self.channels,
                           self.sample, self.depth, bytes(self.order), src_mod, dst_mod) + buf

    def __repr__(self):
        return self.name


def from_view(name, view, sample, depth, order=None):
    """A case out of a numpy view of shape (H, W, C), any strides: its base array is the allocation."""
    base = view
    while base.base is not None:
        base = base.base
    assert base.flags["C_CONTIGUOUS"]
    offset = view.__array_interface__["data"][0] - base.__array_interface__["data"][0]
    h, w, c = view.shape
    return Case(name, base.reshape(-1).view(np.uint8), offset, view.strides, w, h, c, sample, depth, order or tuple(range(c)))


# ---- the model
def offsets(case, order=None, strides=None):
    sy, sx, sc = strides or (case.sy, case.sx, case.sc)
    order = np.asarray((order or case.order)[:case.channels], dtype=np.int64)
    ys = np.arange(case.height, dtype=np.int64)[:, None, None] * sy
    xs = np.arange(case.width, dtype=np.int64)[None, :, None] * sx
    return case.offset + ys + xs + order[None, None, :] * sc


def gather(case, order=None, strides=None, wrap=False):
    """The samples' bits, (H, W, C) uint32, PNG channel k from source channel order[k]."""
    at = offsets(case, order, strides)
    ssz = SAMPLE_BYTES[case.sample]
    if not wrap:
        assert at.min() >= 0 and at.max() + ssz <= len(case.buf), case.name
    raw = np.zeros(at.shape, dtype=np.uint32)
    for b in range(ssz):
        raw |= case.buf.take(at + b, mode="wrap").astype(np.uint32) << np.uint32(8 * b)
    return raw


def to_float32(raw, sample):
    if sample == F16:
        return raw.astype(np.uint16).view(np.float16).astype(np.float32)
    if sample == BF16:
        return (raw << np.uint32(16)).view(np.float32)
    return raw.view(np.float32)


def quantise(raw, sample, depth, wrong=None):
    """The value rule: q = (uint32) clamp(fl32(fl32(x * maxv) + 0.5f), 0, maxv), a NaN 0; integers as they are."""
    if sample in (U8, U16):
        return raw.copy()
    if wrong == "bf16_as_f16" and sample == BF16:
        sample = F16
    x = to_float32(np.ascontiguousarray(raw), sample)
    maxv = np.float32(255.0 if depth == 8 else 65535.0)
    with np.errstate(all="ignore"):
        if wrong == "double":
            a = x.astype(np.float64) * float(maxv) + 0.5
        elif wrong == "no_half":
            a = x * maxv
        elif wrong == "rint":
            a = np.rint(x * maxv)
        else:
            a = x * maxv + np.float32(0.5)
            assert a.dtype == np.float32
        nan = np.isnan(a)
        a = np.where(nan, 0, a)
        if wrong == "no_clamp_above":
            q = np.where(a < 0, 0, np.minimum(a, 2.0 ** 40)).astype(np.int64) & (0xFF if depth == 8 else 0xFFFF)
        else:
            q = np.clip(a, 0, maxv).astype(np.int64)
        if wrong == "nan_not_zero":
            q = np.where(nan, int(maxv), q)
    return q.astype(np.uint32)


def pack(case, wrong=None):
    """The packed image's bytes.  `wrong`: one of WRONG, a model with that mistake."""
    order, strides = None, None
    if wrong == "order_ignored":
        order = tuple(range(4))
    if wrong == "stride_x_packed":
        ssz = SAMPLE_BYTES[case.sample]
        strides = (case.sy, ssz * case.channels if abs(case.sc) == ssz else ssz, case.sc)
    if wrong == "negative_as_positive":
        strides = (abs(case.sy), abs(case.sx), abs(case.sc))
    q = quantise(gather(case, order, strides, wrap=wrong is not None), case.sample, case.depth, wrong)
    if case.depth == 8:
        return q.astype(np.uint8).tobytes()
    return q.astype("<u2" if wrong == "little_endian" else ">u2").tobytes()


WRONG = ("little_endian", "order_ignored", "stride_x_packed", "negative_as_positive", "no_half", "rint", "double", "nan_not_zero",
         "no_clamp_above", "bf16_as_f16")


# ---- data
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def bf16_of(x):
    """float32 -> bfloat16 bits (truncation: any bits do for a test)."""
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def samples(name, shape, sample):
    """Random samples of a type as the array that holds them (BF16: uint16 bits): floats from a little below 0 to a little above 1."""
    rng = _rng(name)
    if sample == U8:
        return rng.integers(0, 256, size=shape, dtype=np.uint8)
    if sample == U16:
        return rng.integers(0, 65536, size=shape, dtype=np.uint16)
    x = rng.uniform(-0.1, 1.1, size=shape).astype(np.float32)
    if sample == F16:
        return x.astype(np.float16)
    if sample == BF16:
        return bf16_of(x)
    return x


def layout_view(arr_hwc_shape, name, sample, layout):
    """Fresh samples for an (H, W, C) image held as HWC or CHW: the (H, W, C) view."""
    h, w, c = arr_hwc_shape
    if layout == "HWC":
        return samples(name, (h, w, c), sample)
    return samples(name, (c, h, w), sample).transpose(1, 2, 0)


# ---- shapes and alignment
def shape_cases():
    out = []
    k = 0
    for w in WIDTHS:
        for h in HEIGHTS:
            for c in (1, 2, 3, 4):
                for layout in ("HWC", "CHW"):
                    sample, depth = COMBOS[k % len(COMBOS)]
                    k += 3   # (coprime to 8: every combination meets every channel count and layout)
                    name = f"shape-{w}x{h}x{c}-{layout}-{SAMPLE_NAMES[sample]}-{depth}"
                    out.append(from_view(name, layout_view((h, w, c), name, sample, layout), sample, depth))
    return out


def combo_cases():
    """Every sample type at every depth, every channel count, both layouts: rows of 67 pixels, so vectors inside a row, across
    a row's end and at an odd phase."""
    out = []
    for sample, depth in COMBOS:
        for c in (1, 2, 3, 4):
            for layout in ("HWC", "CHW"):
                name = f"combo-{SAMPLE_NAMES[sample]}-{depth}-c{c}-{layout}"
                out.append(from_view(name, layout_view((5, 67, c), name, sample, layout), sample, depth))
    # rows that are whole numbers of vectors: the fast paths alone
    for sample, depth in COMBOS:
        for c, layout in ((4, "HWC"), (4, "CHW"), (3, "CHW"), (2, "CHW"), (1, "HWC")):
            name = f"whole-{SAMPLE_NAMES[sample]}-{depth}-c{c}-{layout}"
            out.append(from_view(name, layout_view((3, 96, c), name, sample, layout), sample, depth))
    return out


# ---- layouts
def layout_cases():
    out = []
    for sample, depth in COMBOS:
        t = f"{SAMPLE_NAMES[sample]}-{depth}"
        h, w = 7, 37
        name = f"pitch-{t}"
        out.append(from_view(name, samples(name, (h, w + 11, 4), sample)[:, :w, :], sample, depth))
        name = f"pitch-chw-{t}"
        out.append(from_view(name, samples(name, (3, h, w + 5), sample)[:, :, :w].transpose(1, 2, 0), sample, depth))
        name = f"xstep2-{t}"
        out.append(from_view(name, samples(name, (h, 2 * w, 3), sample)[:, ::2, :], sample, depth))
        name = f"xstep2-chw-{t}"
        out.append(from_view(name, samples(name, (3, h, 2 * w), sample)[:, :, ::2].transpose(1, 2, 0), sample, depth))
        name = f"crop-{t}"
        out.append(from_view(name, samples(name, (h + 9, w + 9, 4), sample)[5:5 + h, 3:3 + w, :], sample, depth))
        name = f"crop-chw-{t}"
        out.append(from_view(name, samples(name, (4, h + 9, w + 9), sample)[:, 4:4 + h, 6:6 + w].transpose(1, 2, 0), sample, depth))
        name = f"bottom-up-{t}"
        out.append(from_view(name, samples(name, (h, w, 4), sample)[::-1], sample, depth))
        name = f"bottom-up-chw-{t}"
        out.append(from_view(name, samples(name, (3, h, w), sample)[:, ::-1, :].transpose(1, 2, 0), sample, depth))
        name = f"mirror-{t}"
        out.append(from_view(name, samples(name, (h, w, 3), sample)[:, ::-1, :], sample, depth))
        name = f"mirror-chw-{t}"
        out.append(from_view(name, samples(name, (3, h, w), sample)[:, :, ::-1].transpose(1, 2, 0), sample, depth))
        name = f"planes-reversed-{t}"
        out.append(from_view(name, samples(name, (3, h, w), sample)[::-1].transpose(1, 2, 0), sample, depth))
        name = f"broadcast-{t}"
        out.append(from_view(name, np.broadcast_to(samples(name, (h, w, 1), sample), (h, w, 3)), sample, depth))
        name = f"bgra-{t}"
        out.append(from_view(name, samples(name, (h, w, 4), sample), sample, depth, order=(2, 1, 0, 3)))
        name = f"bgra-chw-{t}"
        out.append(from_view(name, samples(name, (4, h, w), sample).transpose(1, 2, 0), sample, depth, order=(2, 1, 0, 3)))
        for perm in itertools.permutations(range(3)):
            for layout in ("HWC", "CHW"):
                name = f"perm{''.join(map(str, perm))}-{layout}-{t}"
                out.append(from_view(name, layout_view((h, w, 3), name, sample, layout), sample, depth, order=perm))
    return out


# ---- values
def _plane(name, bits, sample, depth, dtype):
    """A 256 x 256 plane (fewer rows for fewer values, the last row padded with its last value) of one channel."""
    bits = np.asarray(bits, dtype=dtype).reshape(-1)
    rows = max(1, (len(bits) + 255) // 256)
    full = np.concatenate([bits, np.full(rows * 256 - len(bits), bits[-1], dtype=dtype)])
    return from_view(name, full.reshape(rows, 256, 1), sample, depth)


def ties(depth):
    """The three fp32 neighbours either side of every tie (k + 0.5) / maxv, and the tie's own fp32: uint32 bits."""
    maxv = 255 if depth == 8 else 65535
    t = ((np.arange(maxv, dtype=np.float64) + 0.5) / maxv).astype(np.float32).view(np.uint32).astype(np.int64)
    return (t[:, None] + np.arange(-3, 4, dtype=np.int64)[None, :]).reshape(-1).astype(np.uint32)


SPECIAL_F32 = np.array([0x00000000, 0x80000000, 0x3F800000, 0x3F7FFFFF, 0x3F7FFFFE, 0x3F800001, 0x3F800002, 0x40000000, 0x42C80000,
                        0x4B800000, 0x7F7FFFFF, 0xBF800000, 0xBDCCCCCD, 0xB3800000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000,
                        0x7F800001, 0xFFFFFFFF, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x3B808081, 0x3B000000,
                        0x37800080, 0x3F000000, 0x3EFFFFFF, 0x3F000001], dtype=np.uint32)


def value_cases():
    out = []
    allbits = np.arange(65536, dtype=np.uint32)
    for depth in (8, 16):
        out.append(_plane(f"values-f16-all-{depth}", allbits, F16, depth, np.uint16))
        out.append(_plane(f"values-bf16-all-{depth}", allbits, BF16, depth, np.uint16))
        widened = allbits.astype(np.uint16).view(np.float16).astype(np.float32).view(np.uint32)
        out.append(_plane(f"values-f32-f16s-{depth}", widened, F32, depth, np.uint32))
        t = ties(depth)
        for part, start in enumerate(range(0, len(t), 65536)):
            out.append(_plane(f"values-f32-ties-{depth}-{part}", t[start:start + 65536], F32, depth, np.uint32))
        out.append(_plane(f"values-f32-special-{depth}", SPECIAL_F32, F32, depth, np.uint32))
        out.append(_plane(f"values-f32-random-{depth}", _rng(f"bits{depth}").integers(0, 2 ** 32, size=65536, dtype=np.uint32), F32, depth,
                          np.uint32))
    out.append(_plane("values-u16-all", allbits, U16, 16, np.uint16))
    out.append(_plane("values-u8-all", np.arange(256), U8, 8, np.uint8))
    return out


# ---- a batch on the binary search's edges: images of one, two and many tiles, one byte between two large ones
def batch_edge_cases():
    def grey(name, h, w):
        return from_view(name, samples(name, (h, w, 1), U8), U8, 8)
    many = "batch-many-tiles-a"
    return [grey("batch-one-tile", 100, 100), grey("batch-two-tiles", 128, 128),
            from_view(many, samples(many, (4, 256, 256), F32).transpose(1, 2, 0), F32, 8), grey("batch-one-byte", 1, 1),
            from_view("batch-many-tiles-b", samples("batch-many-tiles-b", (256, 256, 3), U16), U16, 16), grey("batch-one-byte-last", 1, 1)]


SHAPES = shape_cases()
COMBO = combo_cases()
LAYOUTS = layout_cases()
VALUES = value_cases()
BATCH_EDGE = batch_edge_cases()
CASES = SHAPES + COMBO + LAYOUTS + VALUES + BATCH_EDGE
SMALL = SHAPES + COMBO + LAYOUTS + BATCH_EDGE   # everything but the value planes
_BY_NAME = {c.name: c for c in CASES}
assert len(_BY_NAME) == len(CASES)


def case(name):
    return _BY_NAME[name]
