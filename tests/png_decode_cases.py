"""The cases of the device PNG decoder (zmx_png_decode_device*, device/zmx_png_decode.h) and a plain reference decoder.

A test-side PNG writer (write_png) takes the rows' filter types as an argument, writes the zlib stream with stored blocks
only — so the files are byte-stable whatever zlib is installed —, splits the IDAT bytes anywhere and puts ancillary chunks
between the other chunks.  The reference decoder (decode_ref) is zlib.decompress plus plain Python over bytes, in both
output modes, with the library's statuses and the order its checks are made in: the chunk walk, the chunks' CRCs, the
stream, its size, the filter bytes, the capacity.  It also notes what a case reaches (the trace): every Paeth choice and tie
by bytewidth, Average sums of nine bits, the filter types on row 0 and on a band's first row.

Pixels in the OWN mode are rows of (width * bpp + 7) / 8 bytes with the padding bits of a row's last byte zero; in the
RGBA8 mode what lodepng_decode32 gives."""
import collections
import functools
import random
import struct
import zlib

(OK, SIGNATURE, IHDR, INTERLACE, CHUNK, CRITICAL, CRC, PLTE, TRNS, STREAM, SIZE, FILTER, CAPACITY) = range(13)
STATUS_NAMES = ["OK", "SIGNATURE", "IHDR", "INTERLACE", "CHUNK", "CRITICAL", "CRC", "PLTE", "TRNS", "STREAM", "SIZE", "FILTER", "CAPACITY"]
OWN, RGBA8 = 0, 1
INFLATE_TRUNCATED, INFLATE_CHECKSUM = 13, 15      # (ZMX_INFLATE_*)
CARRY_BYTES, ENTRIES = 16384, 8                   # (kPngCarryBytes, kPngDecEntries)
LANES = 64

LEGAL = [(0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (2, 8), (2, 16), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (4, 16), (6, 8), (6, 16)]
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
WIDTHS = [1, 2, 3, 7, 8, 9, 63, 64, 65]
HEIGHTS = [1, 2, 63, 64, 65, 129]
SIGNATURE_BYTES = bytes([137, 80, 78, 71, 13, 10, 26, 10])


def bpp_of(colortype, depth):
    return CHANNELS[colortype] * depth


def linebytes_of(width, colortype, depth):
    return (width * bpp_of(colortype, depth) + 7) // 8


def bytewidth_of(colortype, depth):
    return max(1, bpp_of(colortype, depth) // 8)


# ---- the writer
def chunk(kind, data, crc=None):
    if crc is None:
        crc = zlib.crc32(kind + data) & 0xffffffff
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", crc)


def stored_zlib(raw, adler=None):
    """a zlib stream of stored blocks only"""
    out = bytearray(b"\x78\x01")
    pos = 0
    while True:
        piece = raw[pos:pos + 65535]
        pos += len(piece)
        final = pos >= len(raw)
        out += bytes([1 if final else 0]) + struct.pack("<HH", len(piece), len(piece) ^ 0xffff) + piece
        if final:
            break
    out += struct.pack(">I", (zlib.adler32(raw) & 0xffffffff) if adler is None else adler)
    return bytes(out)


def paeth(a, b, c):
    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - c - c)
    if pb < pa:
        a, pa = b, pb
    return c if pc < pa else a


def filter_rows(rows, bytewidth, types):
    """the scanlines of `rows` (bytes each) under the filter types (a type above 4 is written as it is, the row unfiltered)"""
    out = bytearray()
    prev = bytes(len(rows[0])) if rows else b""
    for row, t in zip(rows, types):
        out.append(t)
        line = bytearray(len(row))
        for i, x in enumerate(row):
            a = row[i - bytewidth] if i >= bytewidth else 0
            b = prev[i]
            c = prev[i - bytewidth] if i >= bytewidth else 0
            pred = 0 if t == 0 or t > 4 else a if t == 1 else b if t == 2 else (a + b) >> 1 if t == 3 else paeth(a, b, c)
            line[i] = (x - pred) & 255
        out += line
        prev = row
    return bytes(out)


def write_png(width, height, colortype, depth, rows, types, palette=None, trns=None, splits=None, extra=None, interlace=0, after=b"",
              scanlines=None, deflate=None):
    """rows: `height` bytes objects of linebytes each (the padding bits as given).  palette: bytes of PLTE; trns: bytes of tRNS.
    splits: positions at which the zlib stream is cut into IDATs (a repeated position: an empty IDAT).  extra: a dict of
    lists of whole chunks put "after_ihdr", "before_idat" (behind PLTE and tRNS), "between_idat" (behind the first IDAT) and
    "before_iend".  scanlines: taken in place of the filtered rows.  deflate: a zlib level in place of stored blocks."""
    extra = extra or {}
    if scanlines is None:
        scanlines = filter_rows(rows, bytewidth_of(colortype, depth), types)
    stream = stored_zlib(scanlines) if deflate is None else zlib.compress(scanlines, deflate)
    cuts = [0] + sorted(splits or []) + [len(stream)]
    idats = [chunk(b"IDAT", stream[a:b]) for a, b in zip(cuts, cuts[1:])]
    out = bytearray(SIGNATURE_BYTES)
    out += chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, depth, colortype, 0, 0, interlace))
    for c in extra.get("after_ihdr", []):
        out += c
    if palette is not None:
        out += chunk(b"PLTE", palette)
    if trns is not None:
        out += chunk(b"tRNS", trns)
    for c in extra.get("before_idat", []):
        out += c
    out += idats[0]
    for c in extra.get("between_idat", []):
        out += c
    for c in idats[1:]:
        out += c
    for c in extra.get("before_iend", []):
        out += c
    out += chunk(b"IEND", b"") + after
    return bytes(out)


# ---- the reference decoder
def walk_ref(f):
    """the chunk walk: (status, stop, header dict, entries [(offset, length, crc, kind, index)])"""
    h = dict(width=0, height=0, colortype=0, bitdepth=0, interlace=0, palettesize=0, has_key=0, key_r=0, key_g=0, key_b=0,
             plte=None, trns=b"", known=False)
    if len(f) < 33 or f[:8] != SIGNATURE_BYTES:
        return SIGNATURE, 0, h, []
    if struct.unpack(">I", f[8:12])[0] != 13 or f[12:16] != b"IHDR":
        return IHDR, 0, h, []
    w, hh, bd, ct, comp, filt, il = struct.unpack(">IIBBBBB", f[16:29])
    h.update(width=w, height=hh, colortype=ct, bitdepth=bd, interlace=il)
    if w == 0 or hh == 0 or (ct, bd) not in LEGAL or comp != 0 or filt != 0 or il > 1:
        return IHDR, 0, h, []
    h["known"] = True
    entries = [(8, 13, struct.unpack(">I", f[29:33])[0], "IHDR", 0)]
    pos, index = 33, 1
    while True:
        if len(f) - pos < 12:
            return CHUNK, index, h, entries
        length = struct.unpack(">I", f[pos:pos + 4])[0]
        if length > 0x7fffffff or len(f) - pos - 12 < length:
            return CHUNK, index, h, entries
        kind = f[pos + 4:pos + 8]
        data = f[pos + 8:pos + 8 + length]
        crc = struct.unpack(">I", f[pos + 8 + length:pos + 12 + length])[0]
        if kind == b"IDAT":
            entries.append((pos, length, crc, "IDAT", index))
        elif kind == b"IEND":
            entries.append((pos, length, crc, "IEND", index))
            break
        elif kind == b"PLTE":
            h["palettesize"] = length // 3
            if h["palettesize"] == 0 or h["palettesize"] > 256:
                return PLTE, index, h, entries
            h["plte"] = data
            if ct == 3:
                h["trns"] = b""
            entries.append((pos, length, crc, "PLTE", index))
        elif kind == b"tRNS":
            if ct == 3:
                if length > h["palettesize"]:
                    return TRNS, index, h, entries
                h["trns"] = data
            elif ct == 0:
                if length != 2:
                    return TRNS, index, h, entries
                h.update(has_key=1, key_r=data[0] * 256 + data[1], key_g=data[0] * 256 + data[1], key_b=data[0] * 256 + data[1])
            elif ct == 2:
                if length != 6:
                    return TRNS, index, h, entries
                h.update(has_key=1, key_r=data[0] * 256 + data[1], key_g=data[2] * 256 + data[3], key_b=data[4] * 256 + data[5])
            else:
                return TRNS, index, h, entries
            entries.append((pos, length, crc, "tRNS", index))
        elif not kind[0] & 32:
            return CRITICAL, index, h, entries
        pos += 12 + length
        index += 1
    if ct == 3 and h["plte"] is None:
        return PLTE, index, h, entries
    if il == 1:
        return INTERLACE, index, h, entries
    return OK, index, h, entries


def palette_of(h):
    """the 1024 bytes of the result's palette"""
    out = bytearray(1024)
    if h["plte"] is None:
        return bytes(out)
    for i in range(h["palettesize"]):
        out[4 * i:4 * i + 3] = h["plte"][3 * i:3 * i + 3]
        out[4 * i + 3] = h["trns"][i] if i < len(h["trns"]) else 255
    return bytes(out)


def new_trace():
    return dict(paeth=set(), avg9=set(), row0=set(), seam=set(), first=set())


def unfilter_ref(scan, height, linebytes, bw, trace):
    """the rows, or the first row whose filter byte is above 4"""
    rows = []
    prev = bytes(linebytes)
    for r in range(height):
        t = scan[r * (1 + linebytes)]
        if t > 4:
            return None, r
        line = scan[r * (1 + linebytes) + 1:(r + 1) * (1 + linebytes)]
        rec = bytearray(linebytes)
        if r == 0:
            trace["row0"].add(t)
        elif r % LANES == 0:
            trace["seam"].add(t)
        for i, x in enumerate(line):
            a = rec[i - bw] if i >= bw else 0
            b = prev[i]
            c = prev[i - bw] if i >= bw else 0
            if i < bw and t in (1, 3):
                trace["first"].add(t)
            if t == 0:
                v = x
            elif t == 1:
                v = x + a
            elif t == 2:
                v = x + b
            elif t == 3:
                if a + b >= 256:
                    trace["avg9"].add(bw)
                v = x + ((a + b) >> 1)
            else:
                pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - c - c)
                p = paeth(a, b, c)
                if i >= bw and r > 0:
                    which = "a" if (pa <= pb and pa <= pc) else "b" if pb <= pc else "c"
                    tie = "all" if pa == pb == pc else "ab" if pa == pb else "bc" if pb == pc else "ac" if pa == pc else "none"
                    trace["paeth"].add((bw, which, tie))
                v = x + p
            rec[i] = v & 255
        rows.append(bytes(rec))
        prev = rows[-1]
    return rows, None


def own_pixels(rows, width, colortype, depth):
    bpp = bpp_of(colortype, depth)
    if bpp >= 8 or not rows:
        return b"".join(rows)
    linebytes = len(rows[0])
    valid = width * bpp - 8 * (linebytes - 1)
    mask = (0xff << (8 - valid)) & 0xff
    return b"".join(r[:-1] + bytes([r[-1] & mask]) for r in rows)


def rgba8_pixels(rows, h):
    width, ct, bd = h["width"], h["colortype"], h["bitdepth"]
    pal = palette_of(h)
    out = bytearray()
    for row in rows:
        for x in range(width):
            if bd < 8:
                per = 8 // bd
                v = (row[x // per] >> (8 - bd * (x % per + 1))) & ((1 << bd) - 1)
                if ct == 3:
                    out += pal[4 * v:4 * v + 4] if v < h["palettesize"] else b"\x00\x00\x00\xff"
                else:
                    g = v * 255 // ((1 << bd) - 1)
                    out += bytes([g, g, g, 0 if h["has_key"] and v == h["key_r"] else 255])
                continue
            nb = bd // 8
            px = row[x * CHANNELS[ct] * nb:(x + 1) * CHANNELS[ct] * nb]
            hi = [px[k * nb] for k in range(CHANNELS[ct])]
            full = [int.from_bytes(px[k * nb:(k + 1) * nb], "big") for k in range(CHANNELS[ct])]
            if ct == 0:
                out += bytes([hi[0], hi[0], hi[0], 0 if h["has_key"] and full[0] == h["key_r"] else 255])
            elif ct == 2:
                key = h["has_key"] and full == [h["key_r"], h["key_g"], h["key_b"]]
                out += bytes([hi[0], hi[1], hi[2], 0 if key else 255])
            elif ct == 3:
                out += pal[4 * hi[0]:4 * hi[0] + 4] if hi[0] < h["palettesize"] else b"\x00\x00\x00\xff"
            elif ct == 4:
                out += bytes([hi[0], hi[0], hi[0], hi[1]])
            else:
                out += bytes(hi)
    return bytes(out)


def decode_ref(f, mode, capacity=None, size_only=False):
    """the result as the library gives it: a dict of the result's fields, `pixels` (None unless the status is OK and the
    pixels are stored) and the trace"""
    status, stop, h, entries = walk_ref(f)
    trace = new_trace()
    res = dict(status=status, detail=stop if status in (CHUNK, CRITICAL, PLTE, TRNS) else 0, pixels=None, trace=trace, nentries=len(entries))
    for key in ("width", "height", "colortype", "bitdepth", "interlace", "palettesize", "has_key", "key_r", "key_g", "key_b"):
        res[key] = h[key] if h["known"] else 0
    res["outsize"] = res["outsize_own"] = res["outsize_rgba8"] = 0
    res["palette"] = bytes(1024)
    if not h["known"]:
        return res
    linebytes = linebytes_of(h["width"], h["colortype"], h["bitdepth"])
    res["outsize_own"] = linebytes * h["height"]
    res["outsize_rgba8"] = 4 * h["width"] * h["height"]
    res["outsize"] = res["outsize_rgba8"] if mode == RGBA8 else res["outsize_own"]
    if status in (OK, INTERLACE):
        res["palette"] = palette_of(h)
    if status != OK:
        return res
    for offset, length, crc, _, index in entries:
        if zlib.crc32(f[offset + 4:offset + 8 + length]) & 0xffffffff != crc:
            res.update(status=CRC, detail=index)
            return res
    stream = b"".join(f[o + 8:o + 8 + n] for o, n, _, kind, _ in entries if kind == "IDAT")
    if not stream:
        res.update(status=STREAM, detail=INFLATE_TRUNCATED)
        return res
    want = h["height"] * (1 + linebytes)
    d = zlib.decompressobj()
    try:
        scan = d.decompress(stream)
        ended = d.eof
    except zlib.error as e:
        # (which ZMX_INFLATE_* it is the inflate cases settle; here: the Adler-32, or the stream)
        res.update(status=STREAM, detail=INFLATE_CHECKSUM if "incorrect data check" in str(e) else -1)
        # a stream that is too long is found before its trailer is compared: the size-only run and the capacity say so first
        if res["detail"] == INFLATE_CHECKSUM:
            raw = zlib.decompressobj(-15).decompress(stream[2:])
            if len(raw) != want:
                res.update(status=SIZE, detail=0)
            elif size_only:
                res.update(status=OK, detail=0)
        return res
    if not ended:
        res.update(status=STREAM, detail=INFLATE_TRUNCATED)
        return res
    if len(scan) != want:
        res.update(status=SIZE, detail=0)
        return res
    if size_only:
        return res
    if capacity is not None and res["outsize"] > capacity:
        res["status"] = CAPACITY
        return res
    rows, bad = unfilter_ref(scan, h["height"], linebytes, bytewidth_of(h["colortype"], h["bitdepth"]), trace)
    if rows is None:
        res.update(status=FILTER, detail=bad)
        return res
    res["pixels"] = rgba8_pixels(rows, h) if mode == RGBA8 else own_pixels(rows, h["width"], h["colortype"], h["bitdepth"])
    return res


# ---- the cases
Case = collections.namedtuple("Case", "name file hooks")      # hooks: dict(force_wide=0/1, entry_cap=int)
Bad = collections.namedtuple("Bad", "name file status")


def _case(name, file, force_wide=0, entry_cap=0):
    return Case(name, file, dict(force_wide=force_wide, entry_cap=entry_cap))


def random_rows(rng, width, height, colortype, depth):
    n = linebytes_of(width, colortype, depth)
    return [bytes(rng.randrange(256) for _ in range(n)) for _ in range(height)]


def default_palette(rng, depth, entries=None):
    entries = entries if entries is not None else 1 << depth
    return bytes(rng.randrange(256) for _ in range(3 * entries))


def _image(rng, width, height, colortype, depth, types, **kw):
    rows = kw.pop("rows", None) or random_rows(rng, width, height, colortype, depth)
    if colortype == 3 and "palette" not in kw:
        kw["palette"] = default_palette(rng, depth)
    return write_png(width, height, colortype, depth, rows, types, **kw)


def planted_rows(colortype, depth, height=66, groups=6):
    """Rows of `groups` groups whose neighbourhoods hold Paeth's ties, an Average sum of nine bits and the first-group cases:
    row r - 1 holds (c, b) and row r holds (a, x) in groups 1 and 2, for every byte of the group."""
    bw = bytewidth_of(colortype, depth)
    n = groups * bw
    quads = [(10, 10, 0), (8, 14, 10), (14, 8, 10), (7, 7, 7), (200, 100, 30), (0, 9, 200), (250, 3, 128)]   # (a, b, c)
    rows = [bytearray((17 * r + 3 * i) & 255 for i in range(n)) for r in range(height)]
    for q, (a, b, c) in enumerate(quads):
        for base in (1, LANES - 1):                  # inside a band, and over the seam (rows 63 / 64)
            r = base + 2 * q if base == 1 else base
            g = 1 if base == 1 else 1 + (q % (groups - 2))
            if base != 1 and q >= groups - 2:
                continue
            for k in range(bw):
                rows[r][(g - 1) * bw + k] = c
                rows[r][g * bw + k] = b
                rows[r + 1][(g - 1) * bw + k] = a
                rows[r + 1][g * bw + k] = (a + b + k) & 255
    return [bytes(r) for r in rows]


@functools.lru_cache(maxsize=None)
def filter_cases():
    """per legal pair: each filter type alone and the five cycling from every starting type, on random bytes, over the widths
    and heights"""
    rng = random.Random(20260901)
    out = []
    geometry = [(w, h) for h in HEIGHTS for w in WIDTHS]
    k = 0
    for ct, bd in LEGAL:
        for kind in range(10):
            # (every pair meets a band's last row, the seam and two seams: the cycles take the tall heights in turn)
            w, h = geometry[(7 * k) % len(geometry)]
            if kind >= 5:
                h = (65, 129, 65, 129, 65)[kind - 5]
            k += 1
            types = [kind] * h if kind < 5 else [(kind - 5 + r) % 5 for r in range(h)]
            name = f"ct{ct}_bd{bd}_{w}x{h}_" + (f"type{kind}" if kind < 5 else f"cycle{kind - 5}")
            out.append(_case(name, _image(rng, w, h, ct, bd, types)))
    return out


@functools.lru_cache(maxsize=None)
def planted_cases():
    rng = random.Random(20260902)
    out = []
    # Paeth's ties, Average's ninth bit, the first group: one pair per bytewidth 1, 2, 3, 4, 6, 8, and the low depths
    for ct, bd in [(0, 8), (4, 8), (2, 8), (6, 8), (2, 16), (6, 16), (0, 16), (4, 16), (0, 1), (0, 2), (0, 4), (3, 4)]:
        bw = bytewidth_of(ct, bd)
        rows = planted_rows(ct, bd)
        width = len(rows[0]) * 8 // bpp_of(ct, bd)
        for t in (4, 3, 1, 2):
            out.append(_case(f"planted_ct{ct}_bd{bd}_type{t}", _image(rng, width, len(rows), ct, bd, [t] * len(rows), rows=rows)))
        assert bw in (1, 2, 3, 4, 6, 8)
    # the wide path at a small width
    out.append(_case("forced_wide_rgba8_9x130", _image(rng, 9, 130, 6, 8, [(r + 3) % 5 for r in range(130)]), force_wide=1))
    out.append(_case("forced_wide_grey2_65x65", _image(rng, 65, 65, 0, 2, [(r + 4) % 5 for r in range(65)]), force_wide=1))
    # palettes
    out.append(_case("palette_trns_short", _image(rng, 9, 7, 3, 8, [r % 5 for r in range(7)], palette=default_palette(rng, 8, 200),
                                                  trns=bytes(rng.randrange(256) for _ in range(50)))))
    out.append(_case("palette_index_above_size", _image(rng, 16, 5, 3, 4, [0, 1, 2, 3, 4], palette=default_palette(rng, 4, 5), trns=b"\x00\x80")))
    out.append(_case("palette_of_1", _image(rng, 7, 3, 3, 1, [4, 3, 2], palette=b"\x0a\x14\x1e", trns=b"\x7f")))
    out.append(_case("palette_of_256", _image(rng, 65, 3, 3, 8, [1, 4, 3], palette=default_palette(rng, 8, 256), trns=bytes(range(256)))))
    out.append(_case("palette_in_rgb_file", _image(rng, 3, 3, 2, 8, [0, 1, 2], palette=default_palette(rng, 8, 7))))
    # keys
    for bd in (1, 2, 4, 8, 16):
        rows = random_rows(rng, 9, 4, 0, bd)
        key = rows[1][0] >> (8 - bd) if bd < 8 else rows[1][0] if bd == 8 else rows[1][0] * 256 + rows[1][1]
        if bd == 16:
            rows[2] = rows[1][:1] + bytes([rows[1][1] ^ 1]) + rows[2][2:]     # the key's high byte alone
        out.append(_case(f"key_grey_{bd}", _image(rng, 9, 4, 0, bd, [0, 1, 3, 4], rows=rows, trns=struct.pack(">H", key))))
    for bd in (8, 16):
        rows = random_rows(rng, 5, 4, 2, bd)
        nb = bd // 8
        px = rows[0][:3 * nb]
        key = [int.from_bytes(px[k * nb:(k + 1) * nb], "big") for k in range(3)]
        rows[3] = px + rows[3][3 * nb:]
        if bd == 16:
            rows[2] = px[:5] + bytes([px[5] ^ 0x80]) + rows[2][6:]            # equal in all but one low byte
        out.append(_case(f"key_rgb_{bd}", _image(rng, 5, 4, 2, bd, [2, 4, 1, 3], rows=rows, trns=struct.pack(">HHH", *key))))
    out.append(_case("key_grey_8_out_of_range", _image(rng, 5, 2, 0, 8, [0, 0], trns=b"\x01\x05")))
    # IDAT splits
    rows = random_rows(rng, 9, 5, 6, 8)
    types = [0, 1, 2, 3, 4]
    n = len(stored_zlib(filter_rows(rows, 4, types)))
    for name, cuts in [("single_bytes", list(range(1, n))), ("inside_zlib_header", [1]), ("inside_adler", [n - 2]), ("empty_first", [0]),
                       ("empty_last", [n]), ("empty_middle", [10, 10]), ("more_than_capacity", list(range(5, 5 + 3 * ENTRIES, 3)))]:
        out.append(_case("idat_" + name, write_png(9, 5, 6, 8, rows, types, splits=cuts)))
    out.append(_case("idat_not_adjacent", write_png(9, 5, 6, 8, rows, types, splits=[20], extra={"between_idat": [chunk(b"tEXt", b"k\x00v")]})))
    out.append(_case("idat_rewalk_hook", write_png(9, 5, 6, 8, rows, types, splits=[7, 30]), entry_cap=2))
    # ancillary chunks, with wrong CRCs too; bytes after IEND
    anc = {"after_ihdr": [chunk(b"gAMA", b"\x00\x01\x86\xa0", crc=1)], "before_idat": [chunk(b"tEXt", b"", crc=2), chunk(b"zzZz", b"abc")],
           "before_iend": [chunk(b"tIME", b"1234567", crc=3)]}
    out.append(_case("ancillary_wrong_crcs", write_png(9, 5, 6, 8, rows, types, extra=anc)))
    unknown = {"after_ihdr": [chunk(b"gaMa", b"\x00\x01", crc=1)], "before_idat": [chunk(b"zzZz", b"abc", crc=2)], "before_iend": [chunk(b"teXt", b"", crc=3)]}
    out.append(_case("ancillary_unknown_wrong_crcs", write_png(9, 5, 6, 8, rows, types, extra=unknown)))
    out.append(_case("bytes_after_iend", write_png(9, 5, 6, 8, rows, types, after=b"\x00" * 11 + b"IDAT")))
    # a stream that zlib wrote: dynamic blocks, matches
    rows = [bytes((x * x + r) & 255 for x in range(4 * 64)) for r in range(64)]
    out.append(_case("deflated_rgba8_64x64", write_png(64, 64, 6, 8, rows, [r % 5 for r in range(64)], deflate=9)))
    return out


def valid_cases():
    return filter_cases() + planted_cases()


@functools.lru_cache(maxsize=None)
def malformed_cases():
    rng = random.Random(20260903)
    rows = random_rows(rng, 5, 3, 2, 8)
    types = [1, 2, 4]
    good = write_png(5, 3, 2, 8, rows, types)
    scan = filter_rows(rows, 3, types)
    out = []

    def ihdr(width=5, height=3, depth=8, colortype=2, comp=0, filt=0, il=0, kind=b"IHDR", tail=b""):
        body = chunk(kind, struct.pack(">IIBBBBB", width, height, depth, colortype, comp, filt, il) + tail)
        return SIGNATURE_BYTES + body + good[33:]

    out.append(Bad("signature_byte", b"\x88" + good[1:], SIGNATURE))
    out.append(Bad("shorter_than_33", good[:32], SIGNATURE))
    out.append(Bad("empty_file", b"", SIGNATURE))
    out.append(Bad("ihdr_not_first", ihdr(kind=b"IDHR"), IHDR))
    out.append(Bad("ihdr_length_14", ihdr(tail=b"\x00"), IHDR))
    out.append(Bad("ihdr_width_0", ihdr(width=0), IHDR))
    out.append(Bad("ihdr_height_0", ihdr(height=0), IHDR))
    out.append(Bad("ihdr_rgb_depth_4", ihdr(depth=4), IHDR))
    out.append(Bad("ihdr_colortype_5", ihdr(colortype=5), IHDR))
    out.append(Bad("ihdr_compression_1", ihdr(comp=1), IHDR))
    out.append(Bad("ihdr_filter_1", ihdr(filt=1), IHDR))
    out.append(Bad("ihdr_interlace_2", ihdr(il=2), IHDR))
    # Adam7: a valid interlaced file (1 x 1: one pass, the same scanlines)
    out.append(Bad("interlaced_valid", write_png(1, 1, 0, 8, [b"\x55"], [0], interlace=1), INTERLACE))
    iend = len(good) - 12
    out.append(Bad("chunk_no_iend", good[:iend], CHUNK))
    out.append(Bad("chunk_no_room_for_12", good[:iend] + b"\x00" * 11, CHUNK))
    out.append(Bad("chunk_length_2_31", good[:33] + struct.pack(">I", 0x80000000) + good[37:], CHUNK))
    out.append(Bad("chunk_past_the_end", good[:33] + struct.pack(">I", len(good)) + good[37:], CHUNK))
    out.append(Bad("critical_unknown", good[:33] + chunk(b"IDAx", b"abc") + good[33:], CRITICAL))
    # a wrong CRC on each of the five checked chunk types
    pal = write_png(5, 3, 3, 8, random_rows(rng, 5, 3, 3, 8), types, palette=default_palette(rng, 8, 256), trns=b"\x01\x02")
    spots = {"IHDR": (good, 29), "IDAT": (good, iend - 4), "IEND": (good, len(good) - 4), "PLTE": (pal, 33 + 8 + 768), "tRNS": (pal, 33 + 12 + 768 + 8 + 2)}
    for kind, (f, at) in spots.items():
        out.append(Bad("crc_" + kind, f[:at] + bytes([f[at] ^ 1]) + f[at + 1:], CRC))
    out.append(Bad("plte_missing", write_png(5, 3, 3, 8, rows=[r[:5] for r in rows], types=types), PLTE))
    out.append(Bad("plte_empty", write_png(5, 3, 3, 8, [r[:5] for r in rows], types, palette=b"\x01\x02"), PLTE))
    out.append(Bad("plte_257", write_png(5, 3, 3, 8, [r[:5] for r in rows], types, palette=bytes(3 * 257)), PLTE))
    out.append(Bad("trns_longer_than_plte", write_png(5, 3, 3, 8, [r[:5] for r in rows], types, palette=bytes(9), trns=bytes(4)), TRNS))
    out.append(Bad("trns_before_plte", write_png(5, 3, 3, 8, [r[:5] for r in rows], types, palette=bytes(9),
                                                 extra={"after_ihdr": [chunk(b"tRNS", b"\x01")]}), TRNS))
    out.append(Bad("trns_grey_3_bytes", write_png(5, 3, 0, 8, [r[:5] for r in rows], types, trns=b"\x00\x01\x02"), TRNS))
    out.append(Bad("trns_rgb_2_bytes", write_png(5, 3, 2, 8, rows, types, trns=b"\x00\x01"), TRNS))
    out.append(Bad("trns_grey_alpha", write_png(5, 3, 4, 8, [r[:10] for r in rows], types, trns=b"\x00\x01"), TRNS))
    out.append(Bad("trns_rgba", write_png(5, 3, 6, 8, [r + r[:5] for r in rows], types, trns=b"\x00\x01"), TRNS))
    out.append(Bad("stream_no_idat", good[:33] + good[iend:], STREAM))
    out.append(Bad("stream_idat_empty", good[:33] + chunk(b"IDAT", b"") + good[iend:], STREAM))
    out.append(Bad("stream_bad_zlib_header", good[:33] + chunk(b"IDAT", b"\x78\x02" + stored_zlib(scan)[2:]) + good[iend:], STREAM))
    out.append(Bad("stream_block_type_3", good[:33] + chunk(b"IDAT", b"\x78\x01\x07" + stored_zlib(scan)[3:]) + good[iend:], STREAM))
    out.append(Bad("stream_truncated", good[:33] + chunk(b"IDAT", stored_zlib(scan)[:-5]) + good[iend:], STREAM))
    out.append(Bad("stream_adler", good[:33] + chunk(b"IDAT", stored_zlib(scan, adler=zlib.adler32(scan) ^ 0x100)) + good[iend:], STREAM))
    out.append(Bad("size_one_short", write_png(5, 3, 2, 8, rows, types, scanlines=scan[:-1]), SIZE))
    out.append(Bad("size_one_long", write_png(5, 3, 2, 8, rows, types, scanlines=scan + b"\x00"), SIZE))
    for bad_row in (0, 63, 64):
        tall = random_rows(rng, 3, 66, 0, 8)
        tt = [(r + 2) % 5 for r in range(66)]
        tt[bad_row] = 5
        if bad_row == 0:
            tt[65] = 200        # (the lowest bad row is reported)
        out.append(Bad(f"filter_5_row_{bad_row}", write_png(3, 66, 0, 8, tall, tt), FILTER))
    return out


@functools.lru_cache(maxsize=None)
def truncation_cases():
    """a small file cut at every byte"""
    rng = random.Random(20260904)
    good = write_png(2, 2, 0, 8, random_rows(rng, 2, 2, 0, 8), [1, 4])
    return [Bad(f"cut_at_{n}", good[:n], None) for n in range(len(good))]


# valid here, refused by LodePNG with this error: it checks the CRC of the ancillary chunks it knows, the library skips them
LODEPNG_REFUSES = {"ancillary_wrong_crcs": 57}
FILTER_ROWS = {"filter_5_row_0": 0, "filter_5_row_63": 63, "filter_5_row_64": 64}
