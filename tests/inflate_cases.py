"""Streams for the inflate tests (test_cpu_inflate_cases.py, test_gpu_inflate.py) and a plain-Python reference decoder
that follows device/zmx_inflate.h's rules: its statuses, its outsize / consumed / block, and a trace of what a stream made
it do (block kinds, the longest code used, repeats that crossed the alphabets' boundary, matches that straddled the
ring's wrap or a flush).  Valid streams come from Python's zlib; a small bit writer plants what zlib's encoder never
emits and the malformed ones."""
import functools
import struct
import zlib

GZIP, ZLIB, DEFLATE = 0, 1, 2
WBITS = {GZIP: 31, ZLIB: 15, DEFLATE: -15}
(OK, HEADER, DICT, BLOCK_TYPE, STORED_LEN, TOO_MANY_SYMBOLS, REPEAT, OVERSUBSCRIBED, INCOMPLETE, NO_END_CODE, BAD_CODE, BAD_SYMBOL,
 DISTANCE, TRUNCATED, CAPACITY, CHECKSUM, SIZE) = range(17)
STATUS_NAMES = ["OK", "HEADER", "DICT", "BLOCK_TYPE", "STORED_LEN", "TOO_MANY_SYMBOLS", "REPEAT", "OVERSUBSCRIBED", "INCOMPLETE",
                "NO_END_CODE", "BAD_CODE", "BAD_SYMBOL", "DISTANCE", "TRUNCATED", "CAPACITY", "CHECKSUM", "SIZE"]
# device/zmx_inflate.h (the CPU test holds them against `inflate_print constants`)
RING, STRETCH, LIT_ROOT, DIST_ROOT = 40960, 4096, 10, 8

CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
FIXED_LENS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8 + [5] * 32


# ---------------------------------------------------------------------------------------------- the reference decoder
class _Stop(Exception):
    def __init__(self, status):
        self.status = status


class _Bits:
    def __init__(self, data, pos):
        self.data, self.bit = data, 8 * pos

    def left(self):
        return 8 * len(self.data) - self.bit

    def peek(self, n):
        """the next n bits, the first lowest; zeros behind the end"""
        byte, shift = divmod(self.bit, 8)
        return (int.from_bytes(self.data[byte:byte + 4], "little") >> shift) & ((1 << n) - 1)

    def take(self, n):
        if n > self.left():
            raise _Stop(TRUNCATED)
        v = 0
        if n:
            byte, shift = divmod(self.bit, 8)
            v = (int.from_bytes(self.data[byte:byte + 6], "little") >> shift) & ((1 << n) - 1)
        self.bit += n
        return v


def canonical_codes(lens):
    """symbol -> code (the first bit of the code highest), RFC 1951 3.2.2"""
    count = [0] * 16
    for length in lens:
        count[length] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for length in range(1, 16):
        code = (code + count[length - 1]) << 1
        nxt[length] = code
    codes = {}
    for s, length in enumerate(lens):
        if length:
            codes[s] = nxt[length]
            nxt[length] += 1
    return codes


def _check_counts(lens, kind):
    """InflateCheckCounts"""
    used = [x for x in lens if x]
    if not used:
        return OK if kind == "dist" else INCOMPLETE
    left = 1
    for length in range(1, 16):
        left = (left << 1) - sum(1 for x in used if x == length)
        if left < 0:
            return OVERSUBSCRIBED
    if left > 0 and (kind == "clen" or max(used) != 1):
        return INCOMPLETE
    return OK


class _Code:
    def __init__(self, lens):
        self.by_code = {(length, code): s for s, code in canonical_codes(lens).items() for length in [lens[s]]}
        self.memo = {}

    def symbol(self, bits, trace):
        """InflateSymbol: the canonical walk a bit at a time"""
        window = bits.peek(15)
        found = self.memo.get(window)
        if found is None:
            found = (None, 16)
            code = 0
            for length in range(1, 16):
                code = (code << 1) | ((window >> (length - 1)) & 1)
                s = self.by_code.get((length, code))
                if s is not None:
                    found = (s, length)
                    break
            self.memo[window] = found
        s, length = found
        if length > bits.left():
            raise _Stop(TRUNCATED if bits.left() < 15 else BAD_CODE)
        if s is None:
            raise _Stop(BAD_CODE)
        bits.bit += length
        trace["longest"] = max(trace["longest"], length)
        return s


def _dynamic_lengths(bits, trace):
    v = bits.take(14)
    nlen, ndist, ncode = (v & 31) + 257, ((v >> 5) & 31) + 1, (v >> 10) + 4
    if nlen > 286 or ndist > 30:
        raise _Stop(TOO_MANY_SYMBOLS)
    trace["ncode"].append(ncode)
    clens = [0] * 19
    for i in range(ncode):
        clens[CLEN_ORDER[i]] = bits.take(3)
    status = _check_counts(clens, "clen")
    if status != OK:
        raise _Stop(status)
    code = _Code(clens)
    lens, prev = [], 0
    quiet = {"longest": 0}
    while len(lens) < nlen + ndist:
        s = code.symbol(bits, quiet)
        if s < 16:
            lens.append(s)
            prev = s
            continue
        if s == 16:
            repeat = bits.take(2) + 3
            if not lens:
                raise _Stop(REPEAT)
            value = prev
        elif s == 17:
            repeat, value = bits.take(3) + 3, 0
        else:
            repeat, value = bits.take(7) + 11, 0
        if len(lens) + repeat > nlen + ndist:
            raise _Stop(REPEAT)
        if len(lens) < nlen < len(lens) + repeat:
            trace["crossed"].add(s)
        lens += [value] * repeat
        prev = value
    return lens[:nlen], lens[nlen:]


def _header(fmt, data):
    if fmt == ZLIB:
        if len(data) < 2:
            raise _Stop(TRUNCATED)
        if ((data[0] << 8) | data[1]) % 31 or (data[0] & 15) != 8 or (data[0] >> 4) > 7:
            raise _Stop(HEADER)
        if data[1] & 0x20:
            raise _Stop(DICT)
        return 2
    if fmt == GZIP:
        want = [(0x1f, 0xff), (0x8b, 0xff), (8, 0xff), (0, 0xe0)]
        for i, (value, mask) in enumerate(want):
            if i < len(data) and (data[i] & mask) != value:
                raise _Stop(HEADER)
        if len(data) < 10:
            raise _Stop(TRUNCATED)
        flg, p = data[3], 10
        if flg & 4:
            if len(data) - p < 2:
                raise _Stop(TRUNCATED)
            p += 2 + data[p] + 256 * data[p + 1]
            if p > len(data):
                raise _Stop(TRUNCATED)
        for field in (8, 16):
            if flg & field:
                end = data.find(b"\x00", p)
                if end < 0:
                    raise _Stop(TRUNCATED)
                p = end + 1
        if flg & 2:
            if len(data) - p < 2:
                raise _Stop(TRUNCATED)
            p += 2
        return p
    return 0


def inflate_ref(fmt, data, verify=True):
    """What k_inflate makes of `data`: a dict with the result's fields, `out` (the bytes decoded, up to where it stopped),
    `kernel_status` (before the host's trailer comparison, which `verify` adds: CHECKSUM, SIZE) and the trace."""
    data = bytes(data)
    trace = {"kinds": [], "longest": 0, "crossed": set(), "ncode": [], "wrap": False, "seam": False, "stored_at": [], "end_bit": None}
    r = {"outsize": 0, "consumed": 0, "status": OK, "block": 0, "stored_check": 0, "stored_isize": 0, "trace": trace}
    out = bytearray()
    bits = None
    try:
        bits = _Bits(data, _header(fmt, data))
        while True:
            v = bits.take(3)
            final, kind = v & 1, v >> 1
            trace["kinds"].append(kind)
            if kind == 0:
                trace["stored_at"].append((bits.bit - 3) % 8)
                bits.bit = (bits.bit + 7) // 8 * 8
                v = bits.take(32)
                if (v & 0xffff) != ((v >> 16) ^ 0xffff):
                    raise _Stop(STORED_LEN)
                n, p = v & 0xffff, bits.bit // 8
                if len(data) - p < n:
                    raise _Stop(TRUNCATED)
                out += data[p:p + n]
                bits.bit += 8 * n
            elif kind == 3:
                raise _Stop(BLOCK_TYPE)
            else:
                if kind == 1:
                    litlens, distlens = FIXED_LENS[:288], FIXED_LENS[288:]
                else:
                    litlens, distlens = _dynamic_lengths(bits, trace)
                    if litlens[256] == 0:
                        raise _Stop(NO_END_CODE)
                for lens, what in ((litlens, "lit"), (distlens, "dist")):
                    status = _check_counts(lens, what)
                    if status != OK:
                        raise _Stop(status)
                lit, dist = _Code(litlens), _Code(distlens)
                while True:
                    s = lit.symbol(bits, trace)
                    if s < 256:
                        out.append(s)
                        continue
                    if s == 256:
                        break
                    if s > 285:
                        raise _Stop(BAD_SYMBOL)
                    length = LEN_BASE[s - 257] + bits.take(LEN_EXTRA[s - 257])
                    d = dist.symbol(bits, trace)
                    if d > 29:
                        raise _Stop(BAD_SYMBOL)
                    distance = DIST_BASE[d] + bits.take(DIST_EXTRA[d])
                    if distance > len(out):
                        raise _Stop(DISTANCE)
                    at = len(out)
                    if at % RING + length > RING or (at - distance) % RING + min(length, distance) > RING:
                        trace["wrap"] = True
                    if at % STRETCH + length > STRETCH:
                        trace["seam"] = True
                    if distance >= length:
                        out += out[at - distance:at - distance + length]
                    else:
                        for i in range(length):
                            out.append(out[at - distance + i % distance])
            if final:
                break
            r["block"] += 1
        trace["end_bit"] = bits.bit % 8
        p = (bits.bit + 7) // 8
        need = 8 if fmt == GZIP else 4 if fmt == ZLIB else 0
        bits.bit = 8 * p
        if len(data) - p < need:
            raise _Stop(TRUNCATED)
        if fmt == GZIP:
            r["stored_check"], r["stored_isize"] = struct.unpack("<II", data[p:p + 8])
        elif fmt == ZLIB:
            r["stored_check"] = struct.unpack(">I", data[p:p + 4])[0]
        r["consumed"] = p + need
    except _Stop as stop:
        r["status"] = stop.status
        r["consumed"] = (bits.bit + 7) // 8 if bits is not None else 0
    r["outsize"], r["out"] = len(out), bytes(out)
    r["kernel_status"] = r["status"]
    if verify and r["status"] == OK and fmt != DEFLATE:
        check = zlib.crc32(out) if fmt == GZIP else zlib.adler32(out)
        if check & 0xffffffff != r["stored_check"]:
            r["status"] = CHECKSUM
        elif fmt == GZIP and r["stored_isize"] != len(out) & 0xffffffff:
            r["status"] = SIZE
    return r


def zlib_verdict(fmt, data):
    """(accepted, output, consumed) by zlib's own inflate: accepted only where the stream ends"""
    d = zlib.decompressobj(WBITS[fmt])
    try:
        out = d.decompress(bytes(data))
    except zlib.error:
        return False, None, None
    if not d.eof:
        return False, None, None
    return True, out, len(data) - len(d.unused_data)


# ------------------------------------------------------------------------------------------------------ the bit writer
class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, value, n):
        """n bits of value, the lowest first"""
        self.acc |= (value & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xff)
            self.acc >>= 8
            self.n -= 8
        return self

    def code(self, code, length):
        """a Huffman code: its first bit is its highest"""
        for i in range(length - 1, -1, -1):
            self.bits((code >> i) & 1, 1)
        return self

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)
        return self

    def raw(self, data):
        assert self.n == 0
        self.out += data
        return self

    def bitpos(self):
        return 8 * len(self.out) + self.n

    def bytes(self):
        return bytes(BitWriter.align(self).out)


def length_symbol(length, as_284=False):
    if length == 258 and as_284:
        return 284, 31, 5
    k = max(i for i in range(29) if LEN_BASE[i] <= length and (i == 28 or length < LEN_BASE[i] + (1 << LEN_EXTRA[i])))
    return 257 + k, length - LEN_BASE[k], LEN_EXTRA[k]


def dist_symbol(distance):
    k = max(i for i in range(30) if DIST_BASE[i] <= distance)
    return k, distance - DIST_BASE[k], DIST_EXTRA[k]


def put_symbols(w, litlens, distlens, symbols):
    """symbols: ("lit", byte) | ("match", length, distance[, as_284]) | ("end",) | ("litsym", s) | ("distsym", s)"""
    lit, dist = canonical_codes(litlens), canonical_codes(distlens)
    for sym in symbols:
        if sym[0] == "lit":
            w.code(lit[sym[1]], litlens[sym[1]])
        elif sym[0] == "litsym":
            w.code(lit[sym[1]], litlens[sym[1]])
        elif sym[0] == "distsym":
            w.code(dist[sym[1]], distlens[sym[1]])
        elif sym[0] == "end":
            w.code(lit[256], litlens[256])
        elif sym[0] == "bits":
            w.bits(sym[1], sym[2])
        else:
            s, extra, nextra = length_symbol(sym[1], len(sym) > 3 and sym[3])
            w.code(lit[s], litlens[s]).bits(extra, nextra)
            s, extra, nextra = dist_symbol(sym[2])
            w.code(dist[s], distlens[s]).bits(extra, nextra)
    return w


def fixed_block(w, final, symbols):
    w.bits(final, 1).bits(1, 2)
    return put_symbols(w, FIXED_LENS[:288], FIXED_LENS[288:], list(symbols) + [("end",)])


def stored_block(w, final, data, nlen=None):
    w.bits(final, 1).bits(0, 2).align()
    w.bits(len(data), 16).bits((len(data) ^ 0xffff) if nlen is None else nlen, 16)
    return w.raw(data)


def rle_plan(seq, allow=(16, 17, 18)):
    """the lengths of both alphabets, one after the other, as code-length symbols (symbol, extra bits' value, how many)"""
    plan, i = [], 0
    while i < len(seq):
        run = 1
        while i + run < len(seq) and seq[i + run] == seq[i]:
            run += 1
        if seq[i] == 0 and run >= 11 and 18 in allow:
            take = min(run, 138)
            plan.append((18, take - 11, 7))
        elif seq[i] == 0 and run >= 3 and 17 in allow:
            take = min(run, 10)
            plan.append((17, take - 3, 3))
        elif run >= 4 and 16 in allow:
            take = 1 + min(run - 1, 6)
            plan += [(seq[i], 0, 0), (16, take - 4, 2)]
        else:
            take = 1
            plan.append((seq[i], 0, 0))
        i += take
    return plan


def complete_lengths(k):
    """lengths of a complete prefix code of k >= 2 symbols"""
    m = k.bit_length() - 1
    short = (1 << (m + 1)) - k
    return [m] * short + [m + 1] * (k - short)


def dynamic_header(w, final, litlens, distlens, plan=None, ncode=None, clens=None):
    """a dynamic block's header: `plan` as rle_plan makes it (default: every length on its own), `ncode` code-length code
    lengths sent (default: as few as go), `clens` the code-length code's own lengths (default: a complete code of the symbols
    the plan uses)"""
    w.bits(final, 1).bits(2, 2)
    if plan is None:
        plan = [(v, 0, 0) for v in list(litlens) + list(distlens)]
    if clens is None:
        used = sorted({p[0] for p in plan})
        for filler in (0, 1):          # (the code-length code may not be a single code)
            if len(used) < 2 and filler not in used:
                used = sorted(used + [filler])
        clens = [0] * 19
        for s, length in zip(used, complete_lengths(len(used))):
            clens[s] = length
    if ncode is None:
        ncode = max(4, 1 + max(i for i in range(19) if clens[CLEN_ORDER[i]]))
    w.bits(len(litlens) - 257, 5).bits(len(distlens) - 1, 5).bits(ncode - 4, 4)
    for i in range(ncode):
        w.bits(clens[CLEN_ORDER[i]], 3)
    codes = canonical_codes(clens)
    for s, extra, nextra in plan:
        w.code(codes[s], clens[s]).bits(extra, nextra)
    return w


def dynamic_block(w, final, litlens, distlens, symbols, **kw):
    dynamic_header(w, final, litlens, distlens, **kw)
    return put_symbols(w, litlens, distlens, list(symbols) + [("end",)])


def wrap(fmt, body, out, tail=b""):
    """the deflate data `body` in format fmt's container"""
    if fmt == GZIP:
        return b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03" + body + struct.pack("<II", zlib.crc32(out) & 0xffffffff, len(out) & 0xffffffff) + tail
    if fmt == ZLIB:
        return b"\x78\x9c" + body + struct.pack(">I", zlib.adler32(out) & 0xffffffff) + tail
    return body + tail


# ------------------------------------------------------------------------------------------------------------ the data
@functools.lru_cache(maxsize=None)
def text(n):
    from zopfli_amd.datagen import generate
    return generate("T", n)


@functools.lru_cache(maxsize=None)
def noise(n):
    out, x = bytearray(n), (n * 2654435761 + 12345) & 0xffffffff
    for i in range(n):
        x = (x * 1664525 + 1013904223) & 0xffffffff
        out[i] = x >> 24
    return bytes(out)


def payload(kind, n):
    return bytes(n) if kind == "zeros" else text(n) if kind == "text" else noise(n)


class Case:
    def __init__(self, name, fmt, stream, expect=None, status=OK, **wants):
        self.name, self.fmt, self.stream, self.expect, self.status, self.wants = name, fmt, bytes(stream), expect, status, wants

    def __repr__(self):
        return self.name


SIZES = [0, 1, 257, 65535, 65536, 200000]
VARIANTS = [(0, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY),
            (6, zlib.Z_FIXED), (6, zlib.Z_HUFFMAN_ONLY), (6, zlib.Z_RLE)]
STRATEGY_NAMES = {zlib.Z_DEFAULT_STRATEGY: "default", zlib.Z_FIXED: "fixed", zlib.Z_HUFFMAN_ONLY: "huffman", zlib.Z_RLE: "rle"}


def deflate_with(data, level, strategy, fmt):
    c = zlib.compressobj(level, zlib.DEFLATED, WBITS[fmt], 9, strategy)
    return c.compress(data) + c.flush()


@functools.lru_cache(maxsize=None)
def zlib_cases():
    """Python's zlib at levels 0, 1, 6, 9 and under Z_FIXED, Z_HUFFMAN_ONLY, Z_RLE, wbits -15, 15 and 31, over zeros, text-like
    and random bytes of the six sizes: every combination at the three small sizes; at the three large ones every data and
    variant with the format going round (each format meets each variant and each size)."""
    cases, turn = [], 0
    for kind in ("zeros", "text", "random"):
        for n in SIZES:
            data = payload(kind, n)
            for level, strategy in VARIANTS:
                turn += 1
                for fmt in ((GZIP, ZLIB, DEFLATE) if n <= 257 else ((GZIP, ZLIB, DEFLATE)[turn % 3],)):
                    name = f"zlib_{kind}_{n}_l{level}_{STRATEGY_NAMES[strategy]}_w{WBITS[fmt]}"
                    cases.append(Case(name, fmt, deflate_with(data, level, strategy, fmt), data))
    return cases


def _fifteen_bit_lens():
    # sixteen symbols with lengths 1 .. 14, 15, 15: a complete code
    return list(range(1, 15)) + [15, 15]


@functools.lru_cache(maxsize=None)
def planted_cases():
    cases = []

    def add(name, fmt, body, out, tail=b"", **wants):
        cases.append(Case(name, fmt, wrap(fmt, body, out, tail), out, **wants))

    # ---- a dynamic block whose codes are 15 bits long, literal/length and distance both; the 15-bit ones are used
    # literals 97 .. 109 with 1 .. 13 bits, 110 with 14, the end code and symbol 260 (length 6) with 15; sixteen distance
    # symbols with 1 .. 14, 15, 15 bits, of which number 15 (distances 193 .. 256) is used
    litlens = [0] * 261
    for s, length in zip(list(range(97, 111)) + [256, 260], list(range(1, 15)) + [15, 15]):
        litlens[s] = length
    distlens = _fifteen_bit_lens()
    out = bytearray(97 + i % 14 for i in range(200))
    symbols = [("lit", b) for b in out] + [("match", 6, 198)]
    for i in range(6):
        out.append(out[-198])
    w = dynamic_block(BitWriter(), 1, litlens, distlens, symbols)
    add("dynamic_15_bit_codes", ZLIB, w.bytes(), bytes(out), kinds=[2], longest=15)

    # ---- a distance set of one one-bit code, used
    litlens = [0] * 258
    for s in (65, 66, 256, 257):
        litlens[s] = 2
    w = dynamic_block(BitWriter(), 1, litlens, [1], [("lit", 65), ("lit", 66), ("match", 3, 1), ("match", 3, 1)])
    add("one_bit_distance_code", DEFLATE, w.bytes(), b"AB" + b"B" * 6, kinds=[2])

    # ---- repeats 16 / 17 / 18 that cross from the literal/length lengths into the distance lengths
    litlens = [8] * 192 + [0] * 62 + [4] * 4      # 254 .. 257 (the end code, length 3) with 4 bits, and so the 16 distances
    distlens = [4] * 16
    w = dynamic_block(BitWriter(), 1, litlens, distlens, [("lit", 7), ("lit", 7), ("lit", 7), ("match", 3, 3)], plan=rle_plan(litlens + distlens))
    add("repeat_16_crosses", DEFLATE, w.bytes(), bytes([7]) * 6, kinds=[2], crossed={16})
    for sym, tail, head in ((17, 3, 3), (18, 9, 5)):
        # zeros on both sides of the boundary: `tail` literal/length symbols without a code, `head` distances
        litlens = [0] * (258 + tail)
        litlens[65], litlens[256], litlens[257] = 2, 2, 1
        distlens = [0] * head + [1]
        plan = rle_plan(litlens + distlens, allow=(17,) if sym == 17 else (17, 18))
        w = dynamic_block(BitWriter(), 1, litlens, distlens, [("lit", 65)] * 7 + [("match", 3, DIST_BASE[head])], plan=plan)
        add(f"repeat_{sym}_crosses", DEFLATE, w.bytes(), b"A" * 10, kinds=[2], crossed={sym})

    # ---- HCLEN: eight code-length code lengths (the field holds 4) and all nineteen
    litlens = [8] * 255 + [0, 8]
    w = dynamic_block(BitWriter(), 1, litlens, [0], [("lit", b) for b in b"hclen"], clens=[1 if s in (0, 8) else 0 for s in range(19)], ncode=8)
    add("hclen_field_4", DEFLATE, w.bytes(), b"hclen", kinds=[2], ncode=[8])
    clens = [0] * 19
    for s, length in zip(range(19), [4] * 13 + [5] * 6):
        clens[s] = length
    w = dynamic_block(BitWriter(), 1, litlens, [0], [("lit", b) for b in b"nineteen"], clens=clens, ncode=19)
    add("hclen_19", DEFLATE, w.bytes(), b"nineteen", kinds=[2], ncode=[19])

    # ---- length 258 as symbol 285 and as symbol 284 with extra 31
    for name, as_284 in (("length_258_as_285", False), ("length_258_as_284", True)):
        w = fixed_block(BitWriter(), 1, [("lit", 120), ("match", 258, 1, as_284)])
        add(name, DEFLATE, w.bytes(), b"x" * 259, kinds=[1])

    # ---- distances 1, 2, 63, 64, 65 under lengths 3 and 258; distance 32 768 exactly
    head = text(70)
    symbols, out = [("lit", b) for b in head], bytearray(head)
    for distance in (1, 2, 63, 64, 65):
        for length in (3, 258):
            symbols.append(("match", length, distance))
            for i in range(length):
                out.append(out[-distance])
    add("distances_1_2_63_64_65", GZIP, fixed_block(BitWriter(), 1, symbols).bytes(), bytes(out), kinds=[1])
    far = text(32768)
    w = stored_block(BitWriter(), 0, far)
    fixed_block(w, 1, [("match", 3, 32768), ("match", 258, 32768)])
    add("distance_32768", ZLIB, w.bytes(), far + far[:3] + far[3:261], kinds=[0, 1])

    # ---- stored blocks: none and 65 535 bytes; one that starts at each of the 8 bit positions
    w = stored_block(BitWriter(), 0, b"")
    stored_block(w, 1, noise(65535))
    add("stored_0_and_65535", GZIP, w.bytes(), noise(65535), kinds=[0, 0])
    for k in range(8):
        w, out = BitWriter(), b""
        while w.bitpos() % 8 != k:
            fixed_block(w, 0, [("lit", 200)])     # a nine-bit literal: 19 bits a block
            out += bytes([200])
        stored_block(w, 1, b"stored")
        add(f"stored_at_bit_{k}", DEFLATE, w.bytes(), out + b"stored", stored_at=[k])

    # ---- a final block that ends mid-byte, in front of a trailer
    w = fixed_block(BitWriter(), 1, [("lit", 1)])
    add("final_block_ends_mid_byte", GZIP, w.bytes(), b"\x01", end_bit=2)

    # ---- outputs around one flush stretch and two; matches that straddle the ring's wrap and a flush
    for n in [STRETCH - 2, STRETCH - 1, STRETCH, STRETCH + 1, STRETCH + 2, 2 * STRETCH + 1]:
        data = text(n)
        fmt = (GZIP, ZLIB, DEFLATE)[n % 3]
        cases.append(Case(f"output_of_{n}", fmt, deflate_with(data, 6, zlib.Z_DEFAULT_STRATEGY, fmt), data))
    for name, at, distance, want in (("match_over_flush", STRETCH - 100, 200, {"seam": True}), ("match_over_wrap", RING - 100, 200, {"wrap": True}),
                                     ("match_source_over_wrap", RING + 50, 100, {"wrap": True}), ("match_source_over_wrap_far", RING + 20000, 20100, {"wrap": True})):
        data, w = text(at), BitWriter()
        for start in range(0, at, 60000):
            stored_block(w, 0, data[start:start + 60000])
        fixed_block(w, 1, [("match", 258, distance), ("lit", 33)])
        out = bytearray(data)
        for i in range(258):
            out.append(out[-distance])
        add(name, ZLIB, w.bytes(), bytes(out) + b"!", **want)

    # ---- a gzip header with every optional field at once; bytes behind the trailer; 40 empty blocks in a row
    body = fixed_block(BitWriter(), 1, [("lit", b) for b in b"fields"]).bytes()
    head = b"\x1f\x8b\x08\x1f\x00\x00\x00\x00\x02\x03" + struct.pack("<H", 5) + b"extra" + b"name\x00" + b"a comment\x00"
    head += struct.pack("<H", zlib.crc32(head) & 0xffff)
    cases.append(Case("gzip_every_field", GZIP, head + wrap(GZIP, body, b"fields")[10:], b"fields"))
    for fmt in (GZIP, ZLIB, DEFLATE):
        add(f"trailing_bytes_w{WBITS[fmt]}", fmt, body, b"fields", tail=b"\x1f\x8b\x08trailing")
    w = BitWriter()
    for i in range(40):
        if i % 2:
            stored_block(w, 0, b"")
        else:
            fixed_block(w, 0, [])
    fixed_block(w, 1, [])
    add("forty_empty_blocks", GZIP, w.bytes(), b"", kinds=[1, 0] * 20 + [1])
    return cases


@functools.lru_cache(maxsize=None)
def valid_cases():
    return zlib_cases() + planted_cases()


@functools.lru_cache(maxsize=None)
def malformed_cases():
    """For every status at least one stream, the shortest that reaches it; TRUNCATED also as a text stream cut at each of its
    last 40 bytes."""
    cases = []

    def bad(name, fmt, stream, status):
        cases.append(Case(name, fmt, stream, None, status))

    bad("header_zlib_fcheck", ZLIB, b"\x78\x00", HEADER)
    bad("header_zlib_method", ZLIB, bytes([0x77, (31 - 0x7700 % 31) % 31]), HEADER)
    bad("header_zlib_window", ZLIB, bytes([0x88, (31 - 0x8800 % 31) % 31]), HEADER)
    bad("header_gzip_magic", GZIP, b"\x1f", TRUNCATED)
    bad("header_gzip_magic_wrong", GZIP, b"\x1f\x8c", HEADER)
    bad("header_gzip_method", GZIP, b"\x1f\x8b\x07", HEADER)
    bad("header_gzip_reserved_flag", GZIP, b"\x1f\x8b\x08\x20", HEADER)
    bad("dict", ZLIB, b"\x78\x20", DICT)
    bad("block_type_3", DEFLATE, b"\x07", BLOCK_TYPE)
    bad("stored_len", DEFLATE, b"\x01\x01\x00\x00\x00", STORED_LEN)
    bad("too_many_lengths", DEFLATE, BitWriter().bits(1, 1).bits(2, 2).bits(30, 5).bits(0, 5).bits(0, 4).bytes(), TOO_MANY_SYMBOLS)
    bad("too_many_distances", DEFLATE, BitWriter().bits(1, 1).bits(2, 2).bits(0, 5).bits(30, 5).bits(0, 4).bytes(), TOO_MANY_SYMBOLS)
    # the code-length code { 16: 1 bit, 0: 1 bit }: a repeat first
    w = BitWriter().bits(1, 1).bits(2, 2).bits(0, 5).bits(0, 5).bits(0, 4)
    for s in CLEN_ORDER[:4]:
        w.bits(1 if s in (16, 0) else 0, 3)
    bad("repeat_without_previous", DEFLATE, w.code(1, 1).bits(0, 2).bytes(), REPEAT)
    # { 18: 1 bit, 0: 1 bit }: 138 zeros twice are 276 > 257 + 1
    w = BitWriter().bits(1, 1).bits(2, 2).bits(0, 5).bits(0, 5).bits(0, 4)
    for s in CLEN_ORDER[:4]:
        w.bits(1 if s in (18, 0) else 0, 3)
    bad("repeat_past_the_end", DEFLATE, w.code(1, 1).bits(127, 7).code(1, 1).bits(127, 7).bytes(), REPEAT)
    w = BitWriter().bits(1, 1).bits(2, 2).bits(0, 5).bits(0, 5).bits(0, 4)
    for length in (1, 1, 1, 0):
        w.bits(length, 3)
    bad("oversubscribed_code_lengths_code", DEFLATE, w.bytes(), OVERSUBSCRIBED)
    w = BitWriter().bits(1, 1).bits(2, 2).bits(0, 5).bits(0, 5).bits(0, 4)
    for length in (0, 0, 0, 1):
        w.bits(length, 3)
    bad("incomplete_code_lengths_code", DEFLATE, w.bytes(), INCOMPLETE)
    w = BitWriter().bits(1, 1).bits(2, 2).bits(0, 5).bits(0, 5).bits(0, 4)
    for length in (0, 0, 0, 0):
        w.bits(length, 3)
    bad("empty_code_lengths_code", DEFLATE, w.bytes(), INCOMPLETE)
    litlens = [0] * 257
    litlens[0], litlens[1], litlens[256] = 1, 1, 1
    bad("oversubscribed_lengths", DEFLATE, dynamic_header(BitWriter(), 1, litlens, [0], plan=rle_plan(litlens + [0])).bytes(), OVERSUBSCRIBED)
    litlens = [0] * 257
    litlens[0], litlens[256] = 2, 2
    bad("incomplete_lengths", DEFLATE, dynamic_header(BitWriter(), 1, litlens, [0], plan=rle_plan(litlens + [0])).bytes(), INCOMPLETE)
    litlens = [0] * 257
    litlens[0], litlens[256] = 1, 1
    bad("incomplete_distances", DEFLATE, dynamic_header(BitWriter(), 1, litlens, [2, 2], plan=rle_plan(litlens + [2, 2])).bytes(), INCOMPLETE)
    bad("oversubscribed_distances", DEFLATE, dynamic_header(BitWriter(), 1, litlens, [1, 1, 1], plan=rle_plan(litlens + [1, 1, 1])).bytes(), OVERSUBSCRIBED)
    litlens = [0] * 257
    litlens[0], litlens[1] = 1, 1
    bad("no_end_code", DEFLATE, dynamic_header(BitWriter(), 1, litlens, [0], plan=rle_plan(litlens + [0])).bytes(), NO_END_CODE)
    w = BitWriter().bits(1, 1).bits(2, 2).bits(0, 5).bits(0, 5).bits(0, 4)   # four code-length code lengths: none can be a length but 0
    for length in (2, 2, 2, 2):
        w.bits(length, 3)
    bad("hclen_4_codes", DEFLATE, w.code(3, 2).bits(127, 7).code(3, 2).bits(109, 7).bytes(), NO_END_CODE)   # 18 twice: 138 + 120 zeros
    # a single one-bit code leaves the other bit to no one: sixteen bits of it, so that the input does not end first
    litlens = [0] * 258
    litlens[256], litlens[257] = 1, 1
    w = dynamic_header(BitWriter(), 1, litlens, [1], plan=rle_plan(litlens + [1]))
    put_symbols(w, litlens, [1], [("litsym", 257)])
    bad("bad_distance_code", DEFLATE, w.bits(0xffff, 16).bytes(), BAD_CODE)
    w = dynamic_header(BitWriter(), 1, litlens, [0], plan=rle_plan(litlens + [0]))
    put_symbols(w, litlens, [0], [("litsym", 257)])
    bad("no_distance_code_at_all", DEFLATE, w.bits(0, 16).bytes(), BAD_CODE)
    litlens = [0] * 257
    litlens[256] = 1
    w = dynamic_header(BitWriter(), 1, litlens, [0], plan=rle_plan(litlens + [0]))
    bad("bad_literal_code", DEFLATE, w.bits(0xffff, 16).bytes(), BAD_CODE)
    bad("length_symbol_286", DEFLATE, BitWriter().bits(1, 1).bits(1, 2).code(0b11000110, 8).bytes(), BAD_SYMBOL)
    w = fixed_block_open(BitWriter(), [("lit", 0), ("litsym", 257)])
    bad("distance_symbol_30", DEFLATE, w.code(30, 5).bytes(), BAD_SYMBOL)
    w = fixed_block_open(BitWriter(), [("litsym", 257)])
    bad("distance_before_the_output", DEFLATE, w.code(0, 5).bytes(), DISTANCE)
    w = fixed_block_open(BitWriter(), [("lit", 0), ("lit", 0), ("litsym", 257)])
    bad("distance_one_too_far", DEFLATE, w.code(2, 5).bytes(), DISTANCE)
    bad("empty_deflate", DEFLATE, b"", TRUNCATED)
    bad("empty_zlib", ZLIB, b"", TRUNCATED)
    bad("empty_gzip", GZIP, b"", TRUNCATED)
    bad("stored_without_its_bytes", DEFLATE, b"\x01\x05\x00\xfa\xff1234", TRUNCATED)
    data = text(3000)
    for fmt in (GZIP, ZLIB):
        stream = deflate_with(data, 6, zlib.Z_DEFAULT_STRATEGY, fmt)
        for cut in range(1, 41):
            bad(f"text_w{WBITS[fmt]}_cut_{cut}", fmt, stream[:-cut], TRUNCATED)
    return cases


def fixed_block_open(w, symbols):
    """a final fixed block without its end"""
    w.bits(1, 1).bits(1, 2)
    return put_symbols(w, FIXED_LENS[:288], FIXED_LENS[288:], symbols)


@functools.lru_cache(maxsize=None)
def trailer_cases():
    """what only the trailer comparison finds: a flipped byte in a gzip (and zlib) payload's stored block, a wrong ISIZE"""
    data = noise(1000)
    cases = []
    for fmt in (GZIP, ZLIB):
        stream = bytearray(deflate_with(data, 0, zlib.Z_DEFAULT_STRATEGY, fmt))
        stream[len(stream) // 2] ^= 0x40
        cases.append(Case(f"flipped_stored_byte_w{WBITS[fmt]}", fmt, stream, None, CHECKSUM))
    stream = bytearray(deflate_with(data, 6, zlib.Z_DEFAULT_STRATEGY, GZIP))
    stream[-4] ^= 1
    cases.append(Case("wrong_isize", GZIP, stream, None, SIZE))
    return cases
