"""Piece tables for zmx_bitjoin_device (zopfli_amd/csrc/device/zmx_bitjoin.h) and a plain Python reference.

A case is (name, dst_mod, total_bits, pieces); a piece is (arena_off, src_bit, nbits, dst_bit): bits [src_bit, src_bit +
nbits) of the bit string that begins at byte arena_off of the case's arena (arena_off None: a null pointer, nbits 0) go to
bits [dst_bit, dst_bit + nbits) of the destination.  arena_off mod 16 is the source pointer's address mod 16 (the arena
begins at a 16-byte boundary), dst_mod the destination's.  Bit k of a string is (bytes[k // 8] >> (k % 8)) & 1.  The arena's
bytes are random, so the bits around a piece are there to be masked away.
"""
import numpy as np

TILE = 16384            # kBitjoinTile, bytes
TILE_BITS = 8 * TILE
SIZES = (1, 31, 32, 33, 127, 4099)
OFFSETS = (0, 1, 3, 13)


class Builder:
    """Lays pieces out in one arena: every source in a stretch of its own, 16 bytes of slack on both sides."""

    def __init__(self):
        self.size = 0
        self.pieces = []

    def add(self, src_mod, src_bit, nbits, dst_bit):
        off = (self.size + 31) // 16 * 16 + src_mod
        self.size = off + (src_bit + nbits + 7) // 8 + 16
        self.pieces.append((off, src_bit, nbits, dst_bit))
        return dst_bit + nbits

    def empty(self, dst_bit, null=True):
        self.pieces.append((None if null else 5, 0, 0, dst_bit))

    def case(self, name, dst_mod=0, total_bits=None):
        end = max((p[3] + p[2] for p in self.pieces), default=0)
        return (name, dst_mod, end if total_bits is None else total_bits, list(self.pieces))


def arena_size(pieces):
    return max([off + (sb + nb + 7) // 8 for off, sb, nb, _ in pieces if off is not None and nb] + [0]) + 16


def arena(name, pieces):
    """The case's source bytes: random, the same for the same case name and pieces."""
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) & 0xffffffff
    return np.random.default_rng(seed).integers(0, 256, (arena_size(pieces) + 15) // 16 * 16, dtype=np.uint8)


def expected(total_bits, pieces, arena_bytes):
    """The destination's (total_bits + 7) // 8 bytes, by big-integer shifts."""
    acc = 0
    for off, sb, nb, db in pieces:
        if nb == 0:
            continue
        raw = arena_bytes[off + sb // 8: off + (sb + nb + 7) // 8].tobytes()
        acc |= ((int.from_bytes(raw, "little") >> (sb % 8)) & ((1 << nb) - 1)) << db
    assert acc >> total_bits == 0
    return np.frombuffer(acc.to_bytes((total_bits + 7) // 8, "little"), dtype=np.uint8)


def _pairs(nbits):
    """Every (source bit offset, destination bit offset) mod 32, a piece each, the gaps between them left to be zero."""
    b = Builder()
    cur = 0
    k = 0
    for s in range(32):
        for d in range(32):
            dst = cur + (d - cur) % 32
            cur = b.add((5 * k) % 16, s, nbits, dst)
            k += 1
    return b.case(f"pairs-{nbits}")


def _one_word():
    b = Builder()
    for k in range(32):
        b.add((3 * k) % 16, (7 * k) % 32, 1, 64 + k)
    return b.case("one-word-32", total_bits=128)


def _empties():
    b = Builder()
    b.empty(0)
    b.empty(0, null=False)
    end = b.add(1, 3, 77, 0)
    b.empty(end)
    b.empty(end)
    end = b.add(2, 0, 5000, end)
    b.empty(end + 9, null=False)
    end = b.add(7, 31, 33, end + 9)
    b.empty(end)
    return b.case("empties", dst_mod=3)


def _gaps():
    b = Builder()
    end = b.add(0, 0, 50, 3)      # (and three bits that nothing covers in front of the first piece)
    for gap in range(1, 8):
        end = b.add(gap, gap, 200 + gap, end + gap)
    end = b.add(0, 5, 3000, end + 3)
    end = b.add(9, 2, 40, end + TILE_BITS + 17)       # a gap of more than a whole tile
    end = b.add(4, 0, 6000, end + 2 * TILE_BITS)      # ... and one that holds a whole tile whatever the alignment
    return b.case("gaps", dst_mod=1)


def _tile_edge(e):
    b = Builder()
    end = b.add(3, 1, TILE_BITS + e - 5, 5)                 # ends on, one bit before, one bit after the tile's edge
    end = b.add(6, 9, TILE_BITS, end)                       # begins there, and ends at the next edge likewise
    b.add(11, 30, 777, end + 3)
    return b.case(f"tile-edge{e:+d}")


def _aligned(dst_mod, src_mod):
    b = Builder()
    end = b.add(src_mod, 0, 5000, 0)       # byte-congruent: the straight copy where the offsets agree mod 4
    end = b.add(src_mod, 3, 4100, end)     # ... and a funnel shift
    b.add(src_mod, 8, 8 * 600, end + 8 - end % 8)
    return b.case(f"align-d{dst_mod}-s{src_mod}", dst_mod=dst_mod)


def _tails():
    b = Builder()
    b.add(2, 4, 100, 7)
    return b.case("zero-tail", dst_mod=13, total_bits=100 + 7 + 8 * 37 + 3)


def big():
    """33 MiB + 5 bits from two pieces with odd shifts: the grid-stride loop past 2048 tiles."""
    total = 8 * 33 * (1 << 20) + 5
    first = 8 * 17 * (1 << 20) + 1
    b = Builder()
    end = b.add(1, 3, first, 0)
    b.add(2, 6, total - end, end)
    return b.case("big", dst_mod=3)


def cases():
    out = [_pairs(n) for n in SIZES]
    out += [_one_word(), _empties(), _gaps(), _tails()]
    out += [_tile_edge(e) for e in (-1, 0, 1)]
    out += [_aligned(d, s) for d in OFFSETS for s in OFFSETS]
    out.append(("total-0", 0, 0, []))
    out.append(("total-0-empties", 5, 0, [(None, 0, 0, 0), (None, 0, 0, 0)]))
    b = Builder()
    b.add(5, 6, 1, 0)
    out.append(b.case("total-1", dst_mod=7))
    out.append(("total-1-no-piece", 9, 1, []))
    return out
