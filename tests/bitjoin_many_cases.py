"""Destination tables for zmx_bitjoin_many_device (k_bitjoin_many, zopfli_amd/csrc/device/zmx_bitjoin.h), built from the
piece builder and the big-integer reference of tests/bitjoin_cases.py.

A case is (name, lead, tail, dests, arena_bytes); a destination is (gap, total_bits, pieces), its pieces (arena_off,
src_bit, nbits, dst_bit) as bitjoin_cases.py has them, dst_bit counted from the destination itself.  The destinations lie
in one block that begins at a 16-byte boundary: the first `gap` bytes behind the block's first `lead` bytes, each other
`gap` bytes behind the end of the one before it (0: back to back), `tail` bytes behind the last.  Everything in the block
that is no destination's byte is a canary of 0xA5.
"""
import numpy as np

import bitjoin_cases as bc

TILE = bc.TILE
MAX_BLOCKS = 2048          # kBitjoinMaxBlocks
CANARY = 0xA5


class Many:
    def __init__(self, name, lead, tail=37):
        self.name, self.lead, self.tail = name, lead, tail
        self.b = bc.Builder()
        self.dests = []
        self.at = lead          # where the next destination begins, in the block
        self.k = 0
        self.pending = []       # empty pieces for the destination that comes next

    def dest(self, total_bits, cuts=(), shift=None, gap=0, hole=0):
        """A destination of `total_bits` bits `gap` bytes behind what is there: pieces of the lengths `cuts`, then one to
        the end (`hole`: that many bits in front of every piece but the first are left to be zero; a total of 0 has no
        piece).  shift: source bit address minus destination bit address mod 32 (None: another one for every piece)."""
        self.at += gap
        first = len(self.b.pieces)
        for dst_bit in self.pending:
            self.b.empty(dst_bit)
        self.pending = []
        cur = 0
        lengths = list(cuts)
        while cur < total_bits:
            if cur:
                cur += min(hole, total_bits - cur - 1)
            n = min(lengths.pop(0), total_bits - cur) if lengths else total_bits - cur
            sh = (7 * self.k + 3) % 32 if shift is None else shift
            src_mod = (5 * self.k) % 16
            src_bit = (8 * self.at + cur + sh - 8 * src_mod) % 32
            cur = self.b.add(src_mod, src_bit, n, cur)
            self.k += 1
        self.dests.append((gap, total_bits, self.b.pieces[first:]))
        self.at += (total_bits + 7) // 8
        return self

    def empty_piece(self, dst_bit=0):
        """An empty piece with a null pointer, for the destination that comes next."""
        self.pending.append(dst_bit)
        return self

    def case(self):
        pieces = [p for _, _, ps in self.dests for p in ps]
        return (self.name, self.lead, self.tail, list(self.dests), bc.arena(self.name, pieces))


def shifts(case):
    """(source bit address - destination bit address) mod 32 of every non-empty piece."""
    _, lead, _, dests, _ = case
    out, at = [], lead
    for gap, total_bits, pieces in dests:
        at += gap
        out += [(8 * off + sb - 8 * at - db) % 32 for off, sb, nb, db in pieces if nb]
        at += (total_bits + 7) // 8
    return out


def positions(case):
    """Where every destination begins in the block, and the block's size."""
    _, lead, tail, dests, _ = case
    at, out = lead, []
    for gap, total_bits, _ in dests:
        at += gap
        out.append(at)
        at += (total_bits + 7) // 8
    return out, at + tail


def tiles(case):
    """The tiles of every destination: counted from the 16-byte boundary at or below its own first byte."""
    return [((at % 16) + (tb + 7) // 8 + TILE - 1) // TILE if tb else 0 for at, (_, tb, _) in zip(positions(case)[0], case[3])]


def expected_block(case):
    """The whole block: every destination by big-integer shifts, canaries everywhere else."""
    _, _, _, dests, arena = case
    at, size = positions(case)
    want = np.full(size, CANARY, dtype=np.uint8)
    for a, (_, total_bits, pieces) in zip(at, dests):
        want[a:a + (total_bits + 7) // 8] = bc.expected(total_bits, pieces, arena)
    return want


def cases():
    out = []
    # 5, 1 and 27 bytes back to back from 3 bytes past a 16-byte boundary: neighbours inside one vector
    out.append(Many("neighbours-5-1-27", 3).dest(40).dest(8).dest(8 * 27, cuts=(33, 60)).case())
    # total_bits 0: first, last, two in a row — one of them with empty pieces of its own
    m = Many("empties", 6).dest(0).dest(8 * 9, cuts=(20,)).dest(0)
    m.empty_piece().empty_piece().dest(0)
    out.append(m.dest(300, cuts=(1, 2, 130), hole=2).dest(0).case())
    # exactly one tile, 16-byte aligned; one byte longer; at lead 15 — each with a small neighbour on both sides' far end
    out.append(Many("one-tile", 0).dest(8 * TILE, cuts=(4099, 70001)).dest(8 * 3).case())
    out.append(Many("one-tile-plus-1", 0).dest(8 * (TILE + 1), cuts=(4099, 70001)).dest(8 * 3).case())
    out.append(Many("one-tile-lead-15", 15).dest(8 * TILE, cuts=(4099, 70001)).dest(8 * 3).case())
    # three tiles between destinations of one vector
    out.append(Many("three-tiles-between", 9).dest(8 * 5).dest(8 * (2 * TILE + 100) + 3, cuts=(77, 8 * TILE + 1, 131))
               .dest(8 * 11, cuts=(9,)).case())
    # 2 100 destinations of 20 bytes: more global tiles than the grid has workgroups
    m = Many("many-2100", 5)
    for i in range(2100):
        m.dest(160, cuts=(i % 150 + 1,) if i % 3 else ())
    out.append(m.case())
    # pieces one bit off their destination word, either way, in edge vectors and inside long pieces
    m = Many("one-bit-off", 2)
    for sh in (1, 31):
        m.dest(8 * 40, cuts=(100, 7), shift=sh).dest(8 * 700 + 1, cuts=(3000,), shift=sh)
    out.append(m.case())
    # total_bits no multiple of 8: the last byte's tail is zero and the neighbour's first byte its own
    out.append(Many("ragged-bits", 11).dest(8 * 7 + 3, cuts=(30,)).dest(1).dest(8 * 20 + 7, cuts=(64,), hole=1).dest(8 * 2).case())
    # a gap between destinations, and none around them
    out.append(Many("gaps", 0, tail=0).dest(8 * 30, cuts=(64,)).dest(8 * 30 + 4, gap=1).dest(8 * 33, gap=50).case())
    return out


def table_text(case):
    """The case as tests/hostlib/bitjoin_many_print.cc reads it."""
    _, lead, tail, dests, _ = case
    lines = [f"{lead} {tail} {len(dests)}"]
    for gap, total_bits, pieces in dests:
        lines.append(f"{gap} {total_bits} {len(pieces)}")
        lines += [f"{-1 if off is None else off} {sb} {nb} {db}" for off, sb, nb, db in pieces]
    return "\n".join(lines) + "\n"
