"""The cases of zmx_png_deflate_sizes_device's and ZMX_PNG_FILTER_AUTO's tests (tests/test_cpu_png_trial_cases.py,
tests/test_gpu_png_lodeflate.py, tests/test_gpu_png_auto.py): buffers built to reach the corners of LodePNG's deflate —
its block ends, its window's stale slots, its lazy matching —, histograms of literals built to reach the corners of its
dynamic trees, and images for zopflipng's strategy trials.  What LodePNG and zopflipng make of every one of them is
recorded in tests/golden/png_trials.json by tests/golden/make_png_trials_golden.py."""
import json
import os

import numpy as np

import png_encode_cases as ec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png_trials.json")
WINDOW = 8192          # zopflipng's trials
BLOCK_MIN = 65536      # lodepng_deflatev: blocksize = insize / 8 + 8 within [65536, 262144]


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def blocksize(n):
    return min(262144, max(BLOCK_MIN, n // 8 + 8))


def _rng(name):
    return np.random.default_rng(sum(ord(c) * (i + 1) for i, c in enumerate(name)))


def _noise(name, n, span=256):
    return _rng(name).integers(0, span, n, dtype=np.uint8)


def _zero_heavy(name, n, keep=0.2):
    r = _rng(name)
    a = r.integers(0, 256, n, dtype=np.uint8)
    a[r.random(n) >= keep] = 0
    return a


def _far_copy(name, dist, extra=64):
    """`dist + extra` bytes whose last `extra` repeat the first `extra`: matches at exactly `dist`, if the window has them."""
    a = _noise(name, dist + extra)
    a[dist:] = a[:extra]
    return a


def _across_ends(name):
    """131077 bytes, blocks of 65536: a 5000-byte zero run over the first block end, a 300-byte copy over the second
    (its last five bytes are the third block)."""
    a = _noise(name, 131077)
    a[65536 - 2500:65536 + 2500] = 0
    a[131077 - 300:] = a[20000:20300]
    return a


def _rows_like(name, n):
    """Sub-filtered rows of a smooth RGBA image with a type byte per row."""
    r = _rng(name)
    line = 1 + 4 * 150
    a = r.integers(-2, 3, n).astype(np.int64)
    a[3::4] = 0
    a[::line] = 1
    return (a & 255).astype(np.uint8)


def _lazy_taken(name):
    """A match of 5, and at the next position nothing longer than 6: the first match stands."""
    head = np.frombuffer(b"abcde-Xbcdefy-", dtype=np.uint8)
    return np.concatenate([head, _noise(name, 40, 16) + 100, np.frombuffer(b"abcdefz", dtype=np.uint8)])


def _lazy_beaten(name):
    """A match of 3 ('abc'), and at the next position one of 7 ('bcdefgh'): a literal, then the longer match."""
    return np.frombuffer(b"abcq" + b"bcdefghr" + b"0123456789" + b"abcdefgh" + b"!", dtype=np.uint8).copy()


def _rollback_at_block_end(name, n, end):
    """The three bytes in front of `end` (a block's end, or the buffer's) repeat a trigram 100 bytes before: the match of 3
    is found at end - 3, held back, and taken at end - 2, where nothing can be longer than 2."""
    a = np.arange(n, dtype=np.int64)
    a = ((a * 131 + (a >> 8) * 17 + 7) % 251).astype(np.uint8)   # (no trigram twice within a window)
    a[end - 3:end] = a[end - 103:end - 100]
    return a


def _len3_at(name, dist):
    """Exactly three bytes repeat at `dist`: 4096 is still a match, 4097 a literal (length 3 and offset above 4096)."""
    a = _noise(name, dist + 8, 250)            # (the marker's bytes occur nowhere else)
    a[0:4] = (250, 251, 252, 253)
    a[dist:dist + 3] = (250, 251, 252)
    a[dist + 3] = 7
    return a


# name -> the buffer (uint8); the window of every one is WINDOW
BUFFERS = {
    "one-byte": lambda k: np.array([77], dtype=np.uint8),
    "two-bytes": lambda k: np.array([0, 0], dtype=np.uint8),
    "three-bytes": lambda k: np.array([5, 5, 5], dtype=np.uint8),
    "zeros-258": lambda k: np.zeros(258, dtype=np.uint8),
    "noise-8191": lambda k: _zero_heavy(k, 8191),
    "noise-8192": lambda k: _zero_heavy(k, 8192),
    "noise-8193": lambda k: _zero_heavy(k, 8193),
    "copy-at-8191": lambda k: _far_copy(k, 8191),
    "copy-at-8192": lambda k: _far_copy(k, 8192),
    "copy-at-8193": lambda k: _far_copy(k, 8193),
    "period-8193-x4": lambda k: np.tile(_zero_heavy(k, 8193, 0.6), 4),     # every slot stale by one
    "block-65535": lambda k: _zero_heavy(k, 65535),
    "block-65536": lambda k: _zero_heavy(k, 65536),
    "block-65537": lambda k: _zero_heavy(k, 65537),
    "across-ends-131077": _across_ends,
    "eight-blocks-600000": lambda k: _rows_like(k, 600000),
    "capped-2200000": lambda k: np.concatenate([_rows_like(k, 1200000), _zero_heavy(k, 500000), _noise(k, 500000)]),
    "lazy-taken": _lazy_taken,
    "lazy-beaten": _lazy_beaten,
    "rollback-at-buffer-end": lambda k: _rollback_at_block_end(k, 3000, 3000),
    "rollback-at-block-end": lambda k: _rollback_at_block_end(k, 70000, 65536),
    "len3-at-4096": lambda k: _len3_at(k, 4096),
    "len3-at-4097": lambda k: _len3_at(k, 4097),
    "match-258": lambda k: np.full(600, 7, dtype=np.uint8),
    "hash0-nonzero": lambda k: np.tile(np.array([0x10, 0x01, 0x00], dtype=np.uint8), 3000),
}
BUFFER_IDS = list(BUFFERS)
MIXED_CALL = ["one-byte", "block-65537", "lazy-beaten", "copy-at-8193", "across-ends-131077", "zeros-258", "noise-8192", "match-258"]


def buffer(name):
    return np.ascontiguousarray(BUFFERS[name](name))


def reaches(name):
    """What a buffer case is there for, as facts a test can check without LodePNG."""
    a = buffer(name)
    n = len(a)
    return {"n": n, "blocks": max(1, -(-n // blocksize(n))), "blocksize": blocksize(n)}


# ---- histograms of literals: `use_lz77 0` makes every byte a literal, so a buffer's byte counts are its block's counts
def _from_counts(counts):
    """A buffer (one block: below 65536 bytes) in which byte v occurs counts[v] times, spread evenly."""
    total = int(sum(counts))
    assert 0 < total < BLOCK_MIN
    vals = np.repeat(np.arange(len(counts)), counts).astype(np.uint8)
    return vals[np.argsort((np.arange(total) * 7919) % total, kind="stable")]


def _fib(n, cap):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    assert sum(f[:n]) < cap
    return f[:n]


def _hist_cases():
    out = {}
    out["one-literal"] = [0] * 65 + [300]
    out["two-literals"] = [5, 0, 0, 9]
    out["all-256-flat"] = [7] * 256
    out["all-256-ramp"] = [1 + (v * 37) % 101 for v in range(256)]
    out["fibonacci-22"] = _fib(22, BLOCK_MIN)              # the 15-bit limit: 22 counts want depths up to 21
    out["fibonacci-22-spread"] = [c for f in _fib(22, BLOCK_MIN) for c in (f, 0, 0)]
    out["plateau-ties"] = [3] * 40 + [6] * 20 + [12] * 10 + [24] * 5
    out["plateau-equal-pairs"] = [2, 2, 4, 4, 8, 8, 16, 16, 32, 32, 64, 64]
    # runs of equal code lengths of 3 .. 8 with a breaker between them: the sixes and the rests of LodePNG's run-length coding
    runs = []
    for r in (3, 4, 5, 6, 7, 8, 9, 13):
        runs += [10] * r + [200]
    out["equal-runs-3-8"] = runs
    # zero runs of 138 and 139 between used literals (and 2, 3, 10, 11)
    z = [50] + [0] * 138 + [50] + [0] * 2 + [50] + [0] * 3 + [50] + [0] * 10 + [50] + [0] * 11 + [50]
    out["zero-runs-138"] = z
    out["zero-runs-139"] = [50] + [0] * 139 + [50, 50]
    # few code-length symbols with skewed counts: the 7-bit limit of the code-length code
    cl = []
    for depth_count in (1, 2, 4, 8, 16, 32, 64, 128):
        cl += [max(1, 4096 // depth_count)] * 1
    out["skewed-lengths"] = cl + [1] * 100
    return out


HISTOGRAMS = _hist_cases()
HIST_IDS = list(HISTOGRAMS)


def hist_buffer(name):
    return np.ascontiguousarray(_from_counts(HISTOGRAMS[name]))


# ---- images for zopflipng's trials: (name, width, height, colour type, bit depth)
def _img_shape(case):
    return tuple(case[1:])


def _smooth_rows(w, h, ch, rng):
    """Rows that continue their left neighbour: Sub's ground."""
    step = rng.integers(-1, 2, size=(h, w, ch))
    return (np.cumsum(step, axis=1) * 3 + rng.integers(0, 256, size=(h, 1, ch))) & 255


def _smooth_columns(w, h, ch, rng):
    step = rng.integers(-1, 2, size=(h, w, ch))
    return (np.cumsum(step, axis=0) * 3 + rng.integers(0, 256, size=(1, w, ch))) & 255


def _image(case):
    name, w, h, ct, depth = case
    ch = ec.CHANNELS[ct]
    rng = _rng(name)
    if name.startswith("shape-"):
        return ec.pixels((w, h, ct, depth))
    if name == "all-zero":
        return np.zeros((h, w * ch), dtype=np.uint8)
    if name == "vgrad-w1":
        return ((np.arange(h) * 3) & 255).astype(np.uint8).reshape(h, 1)
    if name == "noise":
        return rng.integers(0, 256, size=(h, w * ch), dtype=np.uint8)
    if name == "smooth-rows":
        return _smooth_rows(w, h, ch, rng).reshape(h, w * ch).astype(np.uint8)
    if name == "smooth-columns":
        return _smooth_columns(w, h, ch, rng).reshape(h, w * ch).astype(np.uint8)
    if name in ("halves", "halves-noisy"):
        a = np.concatenate([_smooth_rows(w, h // 2, ch, rng), _smooth_columns(w, h - h // 2, ch, rng)], axis=0)
        if name == "halves-noisy":
            a[::3] = rng.integers(0, 256, size=a[::3].shape)
        return a.reshape(h, w * ch).astype(np.uint8)
    if name == "plane":
        y, x = np.mgrid[0:h, 0:w]
        a = np.stack([(x * 2 + y * 3 + k * 40 + rng.integers(0, 2, size=(h, w))) & 255 for k in range(ch)], axis=2)
        return a.reshape(h, w * ch).astype(np.uint8)
    if name == "icon-12":
        colors = rng.integers(0, 256, size=(12, 4), dtype=np.uint8)
        colors[:, 3] = 255
        y, x = np.mgrid[0:h, 0:w]
        idx = ((x // 5) * 3 + (y // 7) * 5 + (x * y) % 3) % 12
        return colors[idx].reshape(h, w * 4)
    if name == "hidden-rows":
        # what shows (the rows below) continues the row above; what alpha 0 hides (the rows on top) continues its left
        # neighbour: --lossy_transparent flattens the hidden rows and with them what the trials see
        top = h * 3 // 4
        a = np.concatenate([_smooth_rows(w, top, 4, rng), _smooth_columns(w, h - top, 4, rng)], axis=0).astype(np.uint8)
        a[:top, :, 3] = 0
        a[top:, :, 3] = 255
        return a.reshape(h, w * 4)
    raise KeyError(name)


IMAGES = [("shape-" + ec.shape_id(s),) + tuple(s) for s in ec.SHAPES] + [
    ("all-zero", 32, 16, 6, 8),
    ("vgrad-w1", 1, 200, 0, 8),
    ("noise", 48, 40, 2, 8),
    ("smooth-rows", 120, 40, 2, 8),
    ("smooth-columns", 120, 40, 2, 8),
    ("halves", 120, 60, 2, 8),
    ("halves-noisy", 120, 60, 2, 8),
    ("plane", 90, 50, 6, 8),
    ("icon-12", 40, 40, 6, 8),
    ("hidden-rows", 64, 48, 6, 8),
]
IMAGE_IDS = [c[0] for c in IMAGES]


def image(name):
    """(height, linebytes) uint8 in PNG byte order."""
    case = IMAGES[IMAGE_IDS.index(name)]
    return np.ascontiguousarray(_image(case).astype(np.uint8))


def image_case(name):
    return IMAGES[IMAGE_IDS.index(name)]


def halves_types(h):
    """The predefined types that suit "halves": Sub above, Up below."""
    return np.array([1] * (h // 2) + [2] * (h - h // 2), dtype=np.uint8)


def poor_types(h):
    return np.array([3 if r % 2 else 0 for r in range(h)], dtype=np.uint8)


# (image, predefined types or None): the runs of zmx_png_choose_strategy_device that carry types
PREDEFINED_RUNS = {"halves+suited": ("halves", halves_types), "halves+poor": ("halves", poor_types), "plane+suited": ("plane", lambda h: np.full(h, 4, dtype=np.uint8))}
