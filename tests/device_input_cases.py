"""Inputs for the device-input tests (test_cpu_probe_counts.py, test_gpu_device_input.py): byte patterns at the edges of
the dealing probes (zopfli_amd/csrc/device/zmx_probe.h) and blocks that end in runs of chosen lengths."""
import numpy as np

MASTER_BLOCK = 1000000
# the last probe against `i + 64 <= end` (63 / 64 / 65, 1087 / 1088, 4159 / 4160) and probes at a master-block seam
SEAM_SIZES = [0, 63, 64, 65, 1023, 1087, 1088, 4159, 4160, 999999, 1000000, 1000001, 2000064]


def mixed(n, seed=7):
    """Stretches of 3072 bytes (so that they drift against the 1024 and 4096 strides) of four kinds: random bytes, one
    repeated byte, two to four distinct values, a short period."""
    rng = np.random.default_rng(seed)
    out = np.empty(n + 3072, dtype=np.uint8)
    for at in range(0, n, 3072):
        kind = rng.integers(0, 4)
        if kind == 0:
            seg = rng.integers(0, 256, 3072, dtype=np.uint8)
        elif kind == 1:
            seg = np.full(3072, rng.integers(0, 256), dtype=np.uint8)
        elif kind == 2:
            vals = rng.integers(0, 256, rng.integers(2, 5), dtype=np.uint8)
            seg = vals[rng.integers(0, len(vals), 3072)]
        else:
            seg = np.resize(rng.integers(0, 256, rng.integers(5, 40), dtype=np.uint8), 3072)
        out[at:at + 3072] = seg
    return out[:n].tobytes()


def crafted_probes():
    """One probe every 1024 bytes, each at an edge of the rules.  Returns (bytes, [(is_run, is_few)] per probe)."""
    def pat(values, counts):
        return b"".join(bytes([v]) * c for v, c in zip(values, counts))
    probes = [
        (pat([7, 9], [63, 1]), (0, 1)),                                   # a run of exactly 63: two values, no run
        (pat([9, 7], [1, 63]), (0, 1)),
        (pat([7], [64]), (1, 0)),                                         # a run of exactly 64
        (pat([1, 2, 3, 4], [16, 16, 16, 16]), (0, 1)),                    # exactly 4 distinct values
        (pat([1, 2, 3, 4, 5], [60, 1, 1, 1, 1]), (0, 0)),                 # exactly 5
        (pat([0x01, 0x41, 0x81, 0xC1], [1, 1, 1, 61]), (0, 1)),           # 4 values that differ only in bits 6-7
        (pat([0x01, 0x41, 0x81, 0xC1, 0x02], [15, 15, 15, 15, 4]), (0, 0)),
        (pat([0x3F, 0x7F, 0xBF, 0xFF, 0x3E], [1, 1, 1, 1, 60]), (0, 0)),  # 5, four of them equal in bits 0-5
        (pat([0x80, 0x00], [32, 32]), (0, 1)),
        (pat([0, 255, 0, 255, 0], [10, 10, 10, 10, 24]), (0, 1)),         # values that come back
        (pat([5, 6, 7, 8, 5, 9], [10, 10, 10, 10, 10, 14]), (0, 0)),      # the fifth value late
    ]
    rng = np.random.default_rng(3)
    buf = bytearray(rng.integers(0, 256, 1024 * (len(probes) - 1) + 64, dtype=np.uint8).tobytes())
    for k, (p, _) in enumerate(probes):
        assert len(p) == 64
        buf[1024 * k:1024 * k + 64] = p
    return bytes(buf), [want for _, want in probes]


def runs_threshold(hits, probes=200):
    """`probes` probes of the 4096 stride, the first `hits` of them runs of 64 equal bytes, the others random."""
    rng = np.random.default_rng(11)
    buf = bytearray(rng.integers(0, 256, 4096 * (probes - 1) + 64, dtype=np.uint8).tobytes())
    for k in range(hits):
        buf[4096 * k:4096 * k + 64] = b"\x55" * 64
    return bytes(buf)


def tail_run_start(data, instart, inend):
    """Where the run of bytes equal to data[inend - 1] begins — no lower than instart, and no further than 65600 bytes
    from inend (the walk of PlanReuse, drv_build.h)."""
    r = inend - 1
    while r > instart and inend - r < 65600 and data[r - 1] == data[inend - 1]:
        r -= 1
    return r


TAIL_RUNS = [1, 2, 257, 258, 259, 65599, 65600, 65601]
TAIL_PARENT = 200000


def tail_case(text, run):
    """200 000 bytes of `text` (no zero byte in it) in which a run of `run` zero bytes ends at 150 000, and the child
    blocks of the parent block [0, 200 000).  run = None: the run fills its child block [149 000, 150 000) and goes on
    below it."""
    assert len(text) >= TAIL_PARENT and 0 not in text[:TAIL_PARENT]
    buf = bytearray(text[:TAIL_PARENT])
    end = 150000
    if run is None:
        buf[end - 1500:end] = bytes(1500)
        blocks = [(0, end - 1000), (end - 1000, end), (end, TAIL_PARENT)]
        want = end - 1000
    else:
        buf[end - run:end] = bytes(run)
        blocks = [(0, end), (end, TAIL_PARENT)]
        want = end - min(run, 65600)
    return bytes(buf), blocks, want
