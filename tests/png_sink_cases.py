"""Decoding into strided, planar, float and 16-bit sinks (zmx_png_sink, include/zopfli_amd.h): a plain numpy model of the
value rule — own-mode pixels and their mode to the integer values of each of the 8 output modes (1 .. 4 channels at 8 or
16 bits), from there to each sample type, scattered through a sink's strides — and the cases: files, sinks and refusals.
Nothing here knows the kernel (zopfli_amd/csrc/device/zmx_png_unpack.h); the tile's size is passed in by the tests, which
read it from what tests/hostlib/png_sink_print.cc prints."""
import collections
import functools
import random
import struct

import numpy as np

import png_decode_cases as pc

U8, U16, F16, BF16, F32 = 0, 1, 2, 3, 4   # ZMX_PNG_SAMPLE_*
SAMPLE_BYTES = {U8: 1, U16: 2, F16: 2, BF16: 2, F32: 4}
SAMPLE_NAMES = {U8: "u8", U16: "u16", F16: "f16", BF16: "bf16", F32: "f32"}
# every (sample, bitdepth) a sink may have
COMBOS = ((U8, 8), (U16, 16), (F16, 8), (F16, 16), (BF16, 8), (BF16, 16), (F32, 8), (F32, 16))
MODES = [(c, d) for c in (1, 2, 3, 4) for d in (8, 16)]     # the 8 output modes: channels, bitdepth
FILL = 0xA5                                                  # what a sink's allocation holds before
GUARD = 64
SHAPE = 13                                                   # ZMX_PNG_DECODE_SHAPE
WRONG = ("grey_mean", "key_high_byte", "times_256", "big_endian_u16", "reciprocal", "order_inverse")


# ---- the model: values
@functools.lru_cache(maxsize=None)
def mode_of(file):
    """the mode and the own-mode pixels of a valid file: (dict, bytes)"""
    r = pc.decode_ref(file, pc.OWN)
    assert r["status"] == pc.OK
    return {k: r[k] for k in ("width", "height", "colortype", "bitdepth", "palettesize", "has_key", "key_r", "key_g", "key_b", "palette")}, r["pixels"]


def file_samples(m, own):
    """the file's samples at their own depth, (H, W, channels of the file) uint32"""
    w, h, ct, bd = m["width"], m["height"], m["colortype"], m["bitdepth"]
    ch = pc.CHANNELS[ct]
    rows = np.frombuffer(own, dtype=np.uint8).reshape(h, pc.linebytes_of(w, ct, bd))
    if bd < 8:
        bits = np.unpackbits(rows, axis=1)[:, :w * bd].reshape(h, w, bd).astype(np.uint32)
        weights = (1 << np.arange(bd - 1, -1, -1)).astype(np.uint32)
        return (bits * weights).sum(axis=2, dtype=np.uint32)[:, :, None]
    if bd == 8:
        return rows.reshape(h, w, ch).astype(np.uint32)
    return np.ascontiguousarray(rows).view(">u2").reshape(h, w, ch).astype(np.uint32)


def rgba(m, own, outdepth, wrong=None):
    """lodepng_convert's r, g, b, a of every pixel at `outdepth`, (H, W, 4) uint32"""
    s = file_samples(m, own)
    ct, bd = m["colortype"], m["bitdepth"]
    h, w = s.shape[:2]
    deep = bd == 16 and outdepth == 16
    top = 65535 if deep else 255
    narrow = (lambda v: v) if deep or bd <= 8 else (lambda v: v >> 8)
    key = np.zeros((h, w), dtype=bool)
    if m["has_key"]:
        keys = np.array([m["key_r"], m["key_g"], m["key_b"]], dtype=np.uint32)[:s.shape[2]]
        if wrong == "key_high_byte" and bd == 16:
            key = ((s >> 8) == (keys >> 8)).all(axis=2)
        else:
            key = (s == keys).all(axis=2)
    out = np.empty((h, w, 4), dtype=np.uint32)
    if ct == 3:
        pal = np.zeros((256, 4), dtype=np.uint32)
        pal[:, 3] = 255
        pal[:m["palettesize"]] = np.frombuffer(m["palette"], dtype=np.uint8).reshape(256, 4)[:m["palettesize"]]
        out[:] = pal[s[:, :, 0]]
    elif ct in (0, 4):
        g = s[:, :, 0] * 255 // ((1 << bd) - 1) if bd < 8 else narrow(s[:, :, 0])
        out[:, :, 0] = out[:, :, 1] = out[:, :, 2] = g
        out[:, :, 3] = narrow(s[:, :, 1]) if ct == 4 else np.where(key, 0, top)
    else:
        out[:, :, :3] = narrow(s[:, :, :3])
        out[:, :, 3] = narrow(s[:, :, 3]) if ct == 6 else np.where(key, 0, top)
    if outdepth == 16 and not deep:
        out *= 256 if wrong == "times_256" else 257
    return out


def values(m, own, channels, outdepth, wrong=None):
    """the integer values of the output mode (channels, outdepth), (H, W, channels) uint32, PNG channel order"""
    c = rgba(m, own, outdepth, wrong)
    grey = c[:, :, :3].sum(axis=2, dtype=np.uint32) // 3 if wrong == "grey_mean" else c[:, :, 0]
    if channels == 1:
        return grey[:, :, None].copy()
    if channels == 2:
        return np.stack([grey, c[:, :, 3]], axis=2)
    return c[:, :, :channels].copy()


def lodepng_bytes(v, outdepth):
    """the values as lodepng_convert lays them out: bytes, 16-bit ones high byte first"""
    return v.astype(np.uint8).tobytes() if outdepth == 8 else v.astype(">u2").tobytes()


# ---- the model: samples
def bf16_bits(f):
    """fp32 (>= 0, finite) rounded to nearest-even into bfloat16: the bits"""
    u = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32)
    h, rem = u >> 16, u & 0xffff
    return (h + ((rem > 0x8000) | ((rem == 0x8000) & ((h & 1) == 1)))).astype(np.uint16)


def samples(v, sample, depth, wrong=None):
    """the samples' bytes, (..., ssz) uint8 in memory order"""
    if sample == U8:
        out = v.astype(np.uint8)
    elif sample == U16:
        out = v.astype(">u2" if wrong == "big_endian_u16" else "<u2")
    else:
        maxv = np.float32(255.0 if depth == 8 else 65535.0)
        f = v.astype(np.float32) * (np.float32(1.0) / maxv) if wrong == "reciprocal" else v.astype(np.float32) / maxv
        assert f.dtype == np.float32
        out = f.astype("<f4") if sample == F32 else f.astype("<f2") if sample == F16 else bf16_bits(f).astype("<u2")
    return np.ascontiguousarray(out).view(np.uint8).reshape(v.shape + (SAMPLE_BYTES[sample],))


# ---- sinks
class Sink:
    """An allocation of `buflen` bytes; sample (y, x, c) lies at offset + y * sy + x * sx + c * sc in it."""

    def __init__(self, name, buflen, offset, strides, width, height, channels, sample, depth, order=None):
        self.name, self.buflen, self.offset = name, int(buflen), int(offset)
        self.sy, self.sx, self.sc = (int(s) for s in strides)
        self.width, self.height, self.channels, self.sample, self.depth = width, height, channels, sample, depth
        self.order = tuple(order if order is not None else range(channels)) + (0,) * (4 - channels)

    @property
    def ssz(self):
        return SAMPLE_BYTES[self.sample]

    def offsets(self, wrong=None):
        """where PNG channel k of pixel (y, x) goes: (H, W, C) int64"""
        order = np.asarray(self.order[:self.channels], dtype=np.int64)
        if wrong == "order_inverse":
            order = np.argsort(order)
        ys = np.arange(self.height, dtype=np.int64)[:, None, None] * self.sy
        xs = np.arange(self.width, dtype=np.int64)[None, :, None] * self.sx
        return self.offset + ys + xs + order[None, None, :] * self.sc

    def sample_bytes(self):
        """(H, W, C, ssz) int64: every byte of every sample"""
        return self.offsets()[..., None] + np.arange(self.ssz, dtype=np.int64)

    def expected(self, m, own, wrong=None, before=None):
        """the allocation after the store: FILL (or `before`) with the model's samples scattered into it"""
        buf = np.full(self.buflen, FILL, dtype=np.uint8) if before is None else np.array(before, dtype=np.uint8)
        at = self.offsets(wrong)[..., None] + np.arange(self.ssz, dtype=np.int64)
        assert at.min() >= 0 and at.max() < self.buflen, self.name
        buf[at] = samples(values(m, own, self.channels, self.depth, wrong), self.sample, self.depth, wrong)
        return buf

    def written(self):
        """1 where a byte is a sample's, else 0"""
        n = np.zeros(self.buflen, dtype=np.uint8)
        np.add.at(n, self.sample_bytes().reshape(-1), 1)
        return n

    def record(self, fake=0, base_mod=0):
        return struct.pack("<QQqqqqIIIII4sI", self.buflen, fake, self.offset, self.sy, self.sx, self.sc, self.width, self.height, self.channels,
                           self.sample, self.depth, bytes(self.order), base_mod)

    def __repr__(self):
        return self.name


def _name(sample, depth, channels, layout):
    return f"{SAMPLE_NAMES[sample]}-{depth}-c{channels}-{layout}"


def contiguous(w, h, channels, sample, depth, layout, order=None, lead=0):
    """a tight HWC or CHW tensor `lead` samples into an allocation with guards"""
    ssz = SAMPLE_BYTES[sample]
    strides = (w * channels * ssz, channels * ssz, ssz) if layout == "HWC" else (w * ssz, ssz, w * h * ssz)
    return Sink(_name(sample, depth, channels, layout) + (f"-lead{lead}" if lead else ""), 2 * GUARD + (lead + w * h * channels) * ssz,
                GUARD + lead * ssz, strides, w, h, channels, sample, depth, order)


def layouts(w, h, k):
    """the sinks that are no tight tensor, for a w x h image; k varies the types"""
    sample, depth = COMBOS[k % len(COMBOS)]
    ssz = SAMPLE_BYTES[sample]
    out = []
    # a pitched HWC frame, the pitch no multiple of 16; BGRA on top of it
    pitch = (w * 4 + 3) * ssz + (ssz if ((w * 4 + 3) * ssz) % 16 == 0 else 0)
    out.append(Sink("pitched-bgra-" + SAMPLE_NAMES[sample], 2 * GUARD + pitch * h, GUARD, (pitch, 4 * ssz, ssz), w, h, 4, sample, depth, (2, 1, 0, 3)))
    out.append(Sink("pitched-rgb-" + SAMPLE_NAMES[sample], 2 * GUARD + pitch * h, GUARD, (pitch, 3 * ssz, ssz), w, h, 3, sample, depth))
    # bottom-up, planar and interleaved
    plane = w * h * ssz
    out.append(Sink("bottom-up-chw-" + SAMPLE_NAMES[sample], 2 * GUARD + 3 * plane, GUARD + (h - 1) * w * ssz, (-w * ssz, ssz, plane), w, h, 3, sample, depth))
    out.append(Sink("bottom-up-hwc-" + SAMPLE_NAMES[sample], 2 * GUARD + 2 * plane, GUARD + (h - 1) * w * 2 * ssz, (-w * 2 * ssz, 2 * ssz, ssz), w, h, 2, sample, depth))
    # [::2] in x of a CHW tensor and of an HWC one; mirrored in x
    out.append(Sink("xstep2-chw-" + SAMPLE_NAMES[sample], 2 * GUARD + 6 * plane, GUARD, (2 * w * ssz, 2 * ssz, 2 * plane), w, h, 3, sample, depth))
    out.append(Sink("xstep2-hwc-" + SAMPLE_NAMES[sample], 2 * GUARD + 8 * plane, GUARD, (8 * w * ssz, 8 * ssz, ssz), w, h, 4, sample, depth))
    out.append(Sink("mirror-" + SAMPLE_NAMES[sample], 2 * GUARD + plane, GUARD + (w - 1) * ssz, (w * ssz, -ssz, 0), w, h, 1, sample, depth))
    # a crop inside a larger CHW tensor (W + 11 wide, H + 5 high), planes swapped
    bw, bh = w + 11, h + 5
    out.append(Sink("crop-chw-" + SAMPLE_NAMES[sample], 2 * GUARD + 4 * bw * bh * ssz, GUARD + (2 * bw + 7) * ssz, (bw * ssz, ssz, bw * bh * ssz), w, h, 4,
                    sample, depth, (3, 0, 2, 1)))
    # the planes a row apart: rows interleaved between the planes (planar by the rule)
    out.append(Sink("hcw-" + SAMPLE_NAMES[sample], 2 * GUARD + 3 * plane, GUARD, (3 * w * ssz, ssz, w * ssz), w, h, 3, sample, depth))
    # a base misaligned by 1, 2 and 3 samples
    for lead in (1, 2, 3):
        out.append(contiguous(w, h, 4 if lead == 2 else 3, sample, depth, "HWC" if lead != 3 else "CHW", lead=lead))
        out.append(contiguous(w, h, 1, sample, depth, "CHW", lead=lead))
    return out


# ---- files
File = collections.namedtuple("File", "name file")


def _rows_of(v, ct, bd):
    """rows of a (H, W, ch) integer array at depth 8 or 16"""
    return [np.ascontiguousarray(r).astype(np.uint8 if bd == 8 else ">u2").tobytes() for r in v]


def _random_image(rng, w, h, ct, bd):
    """a file of random pixels whose 16-bit samples' low bytes differ from their high bytes"""
    types = [(r + w) % 5 for r in range(h)]
    kw = {}
    if ct == 3:
        entries = min(1 << bd, 1 + rng.randrange(1 << bd))
        kw["palette"] = pc.default_palette(rng, bd, entries)
        kw["trns"] = bytes(rng.randrange(256) for _ in range(rng.randrange(entries + 1)))
    return pc.write_png(w, h, ct, bd, pc.random_rows(rng, w, h, ct, bd), types, **kw)


@functools.lru_cache(maxsize=None)
def extra_files():
    """what the conversion needs beyond png_decode_cases.valid_cases()"""
    rng = random.Random(20261021)
    out = []
    for ct, bd in pc.LEGAL:                                   # all 15 pairs, a width that is no multiple of a byte's pixels
        out.append(File(f"pair_ct{ct}_bd{bd}_13x5", _random_image(rng, 13, 5, ct, bd)))
    # keys: pixels equal to the key at full depth, and equal in the high byte alone
    for bd in (8, 16):
        top = (1 << bd) - 1
        key = 0x4321 & top
        g = np.array([[key, key ^ 1, key ^ (0x80 if bd == 16 else 0x40), 0, top, key]] * 3, dtype=np.uint32)[:, :, None]
        out.append(File(f"key_grey_{bd}_planted", pc.write_png(6, 3, 0, bd, _rows_of(g, 0, bd), [0, 1, 4], trns=struct.pack(">H", key))))
        kr, kg, kb = 0x1234 & top, 0x5678 & top, 0x9abc & top
        px = [(kr, kg, kb), (kr ^ 1, kg, kb), (kr, kg ^ 2, kb), (kr, kg, kb ^ 4), (kb, kg, kr), (kr, kg, kb), (0, 0, 0)]
        c = np.array([px, px[::-1]], dtype=np.uint32)
        out.append(File(f"key_rgb_{bd}_planted", pc.write_png(7, 2, 2, bd, _rows_of(c, 2, bd), [2, 3], trns=struct.pack(">HHH", kr, kg, kb))))
    # a palette with a short tRNS and indices at and above palettesize
    rows = [bytes((x + 3 * r) % 16 for x in range(19)) for r in range(4)]
    out.append(File("palette_short_trns_above_size", pc.write_png(19, 4, 3, 8, rows, [0, 2, 1, 4], palette=pc.default_palette(rng, 8, 11), trns=b"\x00\x7f\xfe")))
    rows = [bytes(((2 * x) % 16) << 4 | ((2 * x + 1) % 16) for x in range(9)) for _ in range(2)]
    out.append(File("palette4_above_size", pc.write_png(18, 2, 3, 4, rows, [0, 1], palette=pc.default_palette(rng, 4, 6), trns=b"\x10")))
    # low-bit grey at every value of each depth, with a key
    for bd in (1, 2, 4):
        n = 1 << bd
        per = 8 // bd
        width = 2 * n + 1
        vals = [x % n for x in range(width)]
        row = bytearray((width * bd + 7) // 8)
        for x, v in enumerate(vals):
            row[x // per] |= v << (8 - bd * (x % per + 1))
        out.append(File(f"grey_{bd}_every_value", pc.write_png(width, 2, 0, bd, [bytes(row)] * 2, [0, 2], trns=struct.pack(">H", n - 1))))
    # 16-bit samples whose low bytes differ: every channel count
    for ct in (0, 4, 2, 6):
        ch = pc.CHANNELS[ct]
        v = (np.arange(5 * 9 * ch, dtype=np.uint32).reshape(5, 9, ch) * 2731 + 0x00ff) & 0xffff
        out.append(File(f"low_bytes_ct{ct}", pc.write_png(9, 5, ct, 16, _rows_of(v, ct, 16), [1, 2, 3, 4, 0])))
    return out


@functools.lru_cache(maxsize=None)
def shape_files(tile):
    """RGBA8 and RGB16 images at the widths and heights the kernel's geometry turns on; `tile`: a tile's pixels"""
    rng = random.Random(20261022)
    out = []
    shapes = [(w, h) for w in (1, 3, 5, 15, 16, 17, 63, 64, 65) for h in (1, 2)] + [(5, 65), (17, 65), (tile - 1, 1), (tile + 1, 1),
                                                                                    (tile // 2 + 24, 3)]
    for k, (w, h) in enumerate(shapes):
        ct, bd = ((6, 8), (2, 16), (3, 8), (0, 4), (4, 16), (2, 8))[k % 6]
        out.append(File(f"shape_{w}x{h}_ct{ct}_bd{bd}", _random_image(rng, w, h, ct, bd)))
    return out


@functools.lru_cache(maxsize=None)
def all_files():
    """every file the golden covers: the decoder's valid cases (those LodePNG accepts) and the extra ones"""
    return [File(c.name, c.file) for c in pc.valid_cases() if c.name not in pc.LODEPNG_REFUSES] + extra_files()


# ---- the cases: a file and a sink for it
Case = collections.namedtuple("Case", "name file sink")


def _case(f, sink):
    return Case(f.name + ">" + sink.name, f.file, sink)


@functools.lru_cache(maxsize=None)
def cases(tile):
    out = []
    small = [f for f in all_files() if _area(f) <= 70 * 70]
    # every file into two tight tensors whose channels, type and layout go round
    k = 0
    for f in small + shape_files(tile):
        m, _ = mode_of(f.file)
        for _ in range(2):
            sample, depth = COMBOS[k % len(COMBOS)]
            out.append(_case(f, contiguous(m["width"], m["height"], 1 + (k // 3) % 4, sample, depth, ("HWC", "CHW")[(k // 2) % 2])))
            k += 1
    # every channel count, sample type, depth and tight layout, on the shapes
    shapes = shape_files(tile)
    k = 0
    for channels in (1, 2, 3, 4):
        for sample, depth in COMBOS:
            for layout in ("HWC", "CHW"):
                for j in range(3):
                    f = shapes[(5 * k + j * 7) % len(shapes)]
                    m, _ = mode_of(f.file)
                    out.append(_case(f, contiguous(m["width"], m["height"], channels, sample, depth, layout)))
                k += 1
    # the other layouts
    for k, f in enumerate(shapes + extra_files()):
        m, _ = mode_of(f.file)
        for sink in layouts(m["width"], m["height"], k)[k % 3::3] if k >= 8 else layouts(m["width"], m["height"], k):
            out.append(_case(f, sink))
    # (a file may meet the same tight tensor twice: once is enough)
    seen = set()
    return [c for c in out if not (c.name in seen or seen.add(c.name))]


def _area(f):
    m, _ = mode_of(f.file)
    return m["width"] * m["height"]


def batch_nchw(files, sample, depth, channels=3, layout="NCHW"):
    """sinks over ONE allocation: image i of an (N, C, H, W) or (N, H, W, C) tensor; (buflen, [Sink])"""
    m, _ = mode_of(files[0].file)
    w, h = m["width"], m["height"]
    ssz = SAMPLE_BYTES[sample]
    image = channels * w * h * ssz
    strides = (w * ssz, ssz, w * h * ssz) if layout == "NCHW" else (w * channels * ssz, channels * ssz, ssz)
    buflen = 2 * GUARD + len(files) * image
    return buflen, [Sink(f"batch{i}", buflen, GUARD + i * image, strides, w, h, channels, sample, depth) for i in range(len(files))]


# ---- refusals: (sink, what the message holds), one per sentence of the header's list that needs no device
def refusals():
    ok = dict(buflen=0, offset=0, strides=(12, 3, 1), width=4, height=3, channels=3, sample=U8, depth=8)

    def sink(**kw):
        a = dict(ok, **kw)
        s = Sink("refused", a["buflen"], a["offset"], a["strides"], a["width"], a["height"], min(a["channels"], 4), a["sample"], a["depth"], a.get("order"))
        s.channels = a["channels"]
        return s

    return [
        (sink(width=0), "width or height 0"), (sink(height=0), "width or height 0"),
        (sink(channels=0, order=()), "channels"), (sink(channels=5, order=(0, 1, 2, 3)), "channels"),
        (sink(sample=5), "unknown sample type 5"), (sink(depth=4), "bit depth"),
        (sink(sample=U8, depth=16), "not narrowed"), (sink(sample=U16, depth=8, strides=(24, 6, 2)), "not widened"),
        (sink(order=(0, 0, 1)), "permutation"), (sink(order=(0, 1, 3)), "permutation"),
        (sink(sample=F32, strides=(48, 12, 4), offset=2), "multiple of the sample's size"), (sink(sample=F16, strides=(25, 6, 2)), "multiple"),
        # samples that share a byte: a stride of 0, rows that overlap, planes inside a row, samples closer than their size
        (sink(strides=(0, 3, 1)), "share a byte"), (sink(strides=(12, 0, 1)), "share a byte"), (sink(strides=(12, 3, 0)), "share a byte"),
        (sink(strides=(11, 3, 1)), "share a byte"), (sink(strides=(12, 2, 1)), "share a byte"), (sink(strides=(4, 1, 6)), "share a byte"),
        (sink(sample=F32, strides=(48, 12, 2)), "multiple"), (sink(sample=U16, depth=16, strides=(-22, 6, 2)), "share a byte"),
        # 64-bit overflow: a product, a sum, the address below 0
        (sink(height=1 << 31, strides=(1 << 62, 3, 1)), "overflows"), (sink(height=3, width=3, strides=(1 << 62, 1 << 61, 1)), "overflows"),
        (sink(height=2, strides=(-(1 << 41), 3, 1)), "overflows"),
    ]


def accepted():
    """what is no refusal: negative strides, a gap between samples, planes inside a pitch, one row with any stride_y"""
    def sink(strides, w=4, h=3, c=3, sample=U8, depth=8, offset=1 << 20):
        return Sink("fine", 0, offset, strides, w, h, c, sample, depth)
    return [sink((12, 3, 1)), sink((-12, 3, 1)), sink((12, -3, 1)), sink((24, 6, 2)), sink((4, 1, 12)), sink((12, 1, 4)), sink((0, 3, 1), h=1),
            sink((12, 0, 1), w=1), sink((12, 3, 0), c=1), sink((48, 12, 4), sample=F32), sink((5, 1, 64), w=5)]
