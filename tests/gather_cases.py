"""The length and alignment table of zmx_gather_device's tests: tests/test_cpu_gather_rules.py runs it through the
header's rules on the CPU (tests/hostlib/gather_print.cc), tests/test_gpu_gather.py through k_gather.  A case is a
destination offset mod 16 and a list of pieces (source address mod 16, length); byte j of piece i is
(131 i + 7 j + 13) mod 256."""
import random

import numpy as np

TILE = 16384   # zamd::kGatherTile
GUARD = 64     # bytes of 0xA5 on both sides of the destination

LENGTHS = [0, 1, 3, 4, 15, 16, 17, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 5]


def piece_bytes(i, n):
    return ((np.arange(n, dtype=np.int64) * 7 + i * 131 + 13) & 255).astype(np.uint8)


def expected(pieces):
    parts = [piece_bytes(i, n) for i, (_, n) in enumerate(pieces)]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)


def _alignment_pairs():
    """Every (source mod 16, destination mod 16): before each 100-byte piece a filler brings the destination to d."""
    pieces, pos = [], 0
    for s in range(16):
        for d in range(16):
            fill = (d - pos) % 16
            pieces.append(((s + d) % 16, fill))
            pieces.append((s, 100))
            pos += fill + 100
    return pieces


def _small(n, lo, hi, seed):
    rng = random.Random(seed)
    return [(rng.randrange(16), rng.randrange(lo, hi + 1)) for _ in range(n)]


def cases():
    out = []
    out.append(("lengths", 0, [(i % 16, n) for i, n in enumerate(LENGTHS)]))
    out.append(("lengths-reversed", 5, [((3 * i) % 16, n) for i, n in enumerate(reversed(LENGTHS))]))
    for n in LENGTHS:
        out.append((f"alone-{n}", 3, [(1, n)]))
    out.append(("empty-runs", 1, [(0, 0)] * 3 + [(2, 5)] + [(7, 0)] * 2 + [(9, TILE + 7)] + [(0, 0)] * 4 + [(4, 1)] + [(0, 0)] * 3))
    out.append(("alignment-pairs", 0, _alignment_pairs()))
    out.append(("many-in-a-tile", 7, _small(5000, 1, 7, 1)))
    out.append(("across-tiles", 2, [(5, 1), (11, 1000003), (0, 1)]))
    out.append(("tiny-70000", 0, _small(70000, 0, 3, 2)))
    out.append(("none", 0, []))
    out.append(("all-empty", 4, [(3, 0)] * 5))
    return out
