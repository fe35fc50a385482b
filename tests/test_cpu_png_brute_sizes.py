"""The two oracles of tests/test_gpu_png_brute_sizes.py, held to each other on the CPU, and the case set's reach.

LodePNG itself (oracle/_ref/libpng_brute_ref.so, tests/hostlib/png_brute_ref.cc: filterScanline, hash_init, encodeLZ77 and
lodepng_zlib_compress per row and filter type) gives every job of every case of tests/png_brute_size_cases.py its bits,
its bytes and the counters that show what the row reached.  The model of k_png_brute's parallel formulation
(tools/models/png_brute_model.h behind tests/hostlib/png_brute_print.cc, nothing of LodePNG in it) must give the same bits
and bytes.  The model searches at EVERY position, as the kernel does and LodePNG does not, so long rows of zeros or of one
byte at large windows cost it minutes; MODEL_SKIPPED lists the cases it is not given (measured with rows of `flat`: 65 s to
186 s each for the rows around 32768 and of 65537 bytes; 4 s and 12 s for those around 8192), and LodePNG covers those alone.

Six wrong variants of the model (png_brute_print.cc -DPNG_BRUTE_WRONG=1 .. 6) show what comparing sizes and bits buys over
comparing the chosen filter type: three of them change bits and bytes on several cases and the filter type on none;
the other three change nothing that leaves the encoder, for the reasons test_rules_that_no_size_can_see gives.

The program also runs under AddressSanitizer and UBSan, and its `launch` mode holds the driver's launch arithmetic
(zopfli_amd/csrc/host/png_brute_launch.h) to the formulas PngBruteTypes had before the test knobs came."""
import os
import subprocess

import numpy as np
import pytest

import png_brute_size_cases as bc
from zopfli_amd._build import PNG_BRUTE_REF, ROOT

HOSTLIB_DIR = os.path.join(ROOT, "tests", "hostlib")
BUILD = os.path.join(ROOT, "tests", "_build")

# the cases the model is not run on (see above); every other case is
MODEL_SKIPPED = ("beyond-w32768-32767", "beyond-w32768-32768", "beyond-w32768-32769", "beyond-w32768-65537-a", "beyond-w32768-65537-b",
                 "beyond-w8192-8191", "beyond-w8192-8192", "beyond-w8192-16385")
MODELLED = [n for n in bc.CASE_IDS if bc.CASES[n].model]

# (variant, what is wrong, cases that must tell it from LodePNG)
WRONG_SEEN = [
    (1, "maxlazymatch 258 at every window", ("lazy-switch-w4096", "sweep-w4096-5000", "beyond-w2048-4097")),
    (3, "the length-3 / offset > 4096 rule dropped", ("far3-w8192", "far3-w32768", "sweep-w8192-5000", "job-loop")),
    (6, "nicematch ignored", ("beyond-w256-513", "beyond-w2048-2049", "chunk-1024", "sweep-w8192-5000")),
]
WRONG_UNSEEN = [
    (2, "the zero count capped at 257"),
    (4, "the tail hash shifted by 4 instead of 8"),
    (5, 'every "keep" link resolved to the slot itself'),
]
UNSEEN_CASES = ("chunk-seam-keys-w512", "chunk-2049", "beyond-w256-513", "beyond-w2048-4097", "sweep-w8-5000", "sweep-w64-5000", "sweep-w8192-5000",
                "one-pixel-bw3", "tiny-2", "tiny-3", "tiny-5", "job-loop")


def _make(*args):
    subprocess.check_call(["make", "-s", "-C", HOSTLIB_DIR, "-f", "png_brute.mk"] + list(args))


@pytest.fixture(scope="module")
def exe():
    _make()
    return os.path.join(BUILD, "png_brute_print")


@pytest.fixture(scope="module")
def ref():
    if not os.path.exists(PNG_BRUTE_REF):
        pytest.skip("oracle/_ref/libpng_brute_ref.so not built (the reference's tree is not at hand)")
    return bc.ref_library(PNG_BRUTE_REF)


@pytest.mark.parametrize("name", bc.CASE_IDS)
def test_cases_reach_what_they_are_for(ref, name):
    case = bc.CASES[name]
    _, _, reach, _ = bc.ref_run(ref, case)
    case.check(reach)


def test_the_lists_are_used():
    cases = bc.CASES.values()
    assert set(MODEL_SKIPPED) == {c.name for c in cases if not c.model}
    assert {c.window for c in cases} >= {1, 2, 4, 8, 64, 256, 2048, 4096, 8192, 16384, 32768}
    assert {c.bytewidth for c in cases} == {1, 2, 3, 4, 6, 8}
    lengths = {(c.linebytes, c.window) for c in cases}
    for w in (256, 2048, 8192, 32768):
        assert {(w - 1, w), (w, w), (w + 1, w), (2 * w + 1, w)} <= lengths
    for n in (bc.LDS_LAST, bc.LDS_LAST + 1, bc.LDS_DEFAULT_LAST, bc.LDS_DEFAULT_LAST + 1):
        assert {(n, 2048), (n, 32768)} <= lengths
    assert {n for n, _ in lengths} >= {1, 2, 3, 1023, 1024, 1025, 2049}
    assert any(c.linebytes == c.bytewidth for c in cases)
    for w in bc.SWEEP_WINDOWS:
        for n in (300, 5000):
            assert bc.CASES[f"sweep-w{w}-{n}"].kinds == bc.KINDS
    # every kind of row at rows beyond zopflipng's window
    long_kinds = {k for c in cases if c.window == 32768 and c.linebytes > 32768 for k in c.kinds}
    assert {"flat-rare", "zero-runs", "periodic", "edge"} <= long_kinds
    # the knobs: the scratch path for every short case, the job loop on 1, 2, 3 workgroups and the driver's own grid
    for c in cases:
        assert ((1, 0) in c.knobs) == (c.linebytes <= bc.FORCE_SCRATCH_MAX) and c.knobs[0] == (0, 0)
    loop = bc.CASES["job-loop"]
    assert [g for f, g in loop.knobs if f == 0] == [0, 1, 2, 3] and loop.height * 5 > 3
    assert loop.kinds[2:4] == ("zeros", "random") and loop.kinds[4:6] == ("byte-85", "gradient") and loop.linebytes == 5000


@pytest.mark.parametrize("name", bc.CASE_IDS)
def test_lodepngs_bytes_are_its_bits_rounded(ref, name):
    """lodepng_zlib_compress' length is 2 + ceil((3 + data + 7) / 8) + 4 of encodeLZ77's symbols under the fixed code, for
    every job; and filter() with LFS_BRUTE_FORCE picks the first smallest of a row's five."""
    size, bits, _, types = bc.ref_run(ref, bc.CASES[name])
    assert np.array_equal(size, 6 + (bits + 7) // 8), bc.mismatches(size, 6 + (bits + 7) // 8)
    assert np.array_equal(types, bc.first_smallest(size))


@pytest.mark.parametrize("name", MODELLED)
def test_model_is_lodepng(exe, ref, tmp_path, name):
    case = bc.CASES[name]
    size, bits, _, _ = bc.ref_run(ref, case)
    got_size, got_bits = bc.model_run(exe, tmp_path, case)
    assert np.array_equal(got_bits, bits), ("bits (row, type, model, LodePNG)", bc.mismatches(got_bits, bits))
    assert np.array_equal(got_size, size), ("bytes (row, type, model, LodePNG)", bc.mismatches(got_size, size))


@pytest.mark.parametrize("variant,what,names", WRONG_SEEN, ids=[f"wrong{v}" for v, _, _ in WRONG_SEEN])
def test_wrong_models_are_told_apart(ref, tmp_path, variant, what, names):
    """A model with one rule wrong differs from LodePNG in bits on every case named for it — and in the filter type on
    none of them: the comparison tests/test_gpu_png_brute.py makes would have passed it."""
    _make(f"WRONG={variant}", f"SUFFIX=_wrong{variant}")
    wrong = os.path.join(BUILD, f"png_brute_print_wrong{variant}")
    for name in names:
        case = bc.CASES[name]
        size, bits, _, types = bc.ref_run(ref, case)
        got_size, got_bits = bc.model_run(wrong, tmp_path, case)
        nbits, nbytes = int((got_bits != bits).sum()), int((got_size != size).sum())
        ntypes = int((bc.first_smallest(got_size) != types).sum())
        print(f"wrong {variant} ({what}) on {name}: {nbits} jobs differ in bits, {nbytes} in bytes, {ntypes} rows in the filter type")
        assert nbits > 0 and nbytes > 0, (what, name)
        assert ntypes == 0, (what, name, "the types tell it too: say so in the docstring")


@pytest.mark.parametrize("variant,what", WRONG_UNSEEN, ids=[f"wrong{v}" for v, _ in WRONG_UNSEEN])
def test_rules_that_no_size_can_see(ref, tmp_path, variant, what):
    """Three rules of the formulation that no output of the encoder depends on, so no comparison of sizes can hold the
    kernel to them; this test records that, and fails when a case is found that does tell one of them.
      zero count capped at 257   the count only skips zeros the comparison would walk over, and picks the zero-run chain
                                 when `length > numzeros`; at 257 and 258 alike the first candidate inside the run gives
                                 258 >= nicematch and ends the search.
      tail hash shifted by 4     the last two positions can only match 2 and 1 bytes, which is a literal whatever the
                                 search finds, and nothing is inserted after them.
      "keep" resolved to itself  a link keeps what its slot held only when its key was never seen in the row, so no earlier
                                 position has that hash: a walk that arrives there ends — on `chain[i] == i` when the slot
                                 holds itself, on the stale hash or on an offset that goes backwards when it holds what
                                 position p - W wrote — before anything is compared."""
    _make(f"WRONG={variant}", f"SUFFIX=_wrong{variant}")
    wrong = os.path.join(BUILD, f"png_brute_print_wrong{variant}")
    for name in UNSEEN_CASES:
        case = bc.CASES[name]
        size, bits, _, _ = bc.ref_run(ref, case)
        got_size, got_bits = bc.model_run(wrong, tmp_path, case)
        assert np.array_equal(got_bits, bits) and np.array_equal(got_size, size), (what, name, bc.mismatches(got_bits, bits))


def _parent_launch(n, jobs):
    """PngBruteTypes' launch as the driver computed it before it took knobs, restated."""
    row = bc.row_bytes(n)
    in_lds = row <= 148 * 1024
    stride = (65536 * 4 + 4 * n + (0 if in_lds else row) + 255) & ~255
    per_cu = max(1, min(2, (160 * 1024) // (row + 12 * 1024))) if in_lds else 1
    grid = max(1, min(jobs, 256 * per_cu, (1 << 30) // stride))
    return [int(in_lds), int(in_lds and row > 64 * 1024), row, stride, grid, row if in_lds else 0]


def _launches(exe, force, cap, pairs):
    out = subprocess.run([exe, "launch", str(force), str(cap)] + [str(v) for p in pairs for v in p], capture_output=True, text=True, check=True)
    return [[int(v) for v in line.split()] for line in out.stdout.splitlines()]


def test_launch_is_the_parents_without_knobs(exe):
    """Grid, dynamic LDS, scratch stride, the LDS / scratch choice and the attribute call of the default knobs, which the
    three production callers pass, over row lengths around every threshold and job counts around every cap; and what the
    knobs change: force_scratch takes the scratch path's numbers at any length, max_workgroups only lowers the grid."""
    lengths = sorted({1, 2, 3, 255, 1000, 4096, 5000, 6143, 6144, 6145, 7281, 7282, 8192, 16383, 16384, 16838, 16839, 16840, 16841, 32768, 65537,
                      100000, 1 << 20, (1 << 22) - 1, 1 << 24, 123456789, 0x7fffffff} | {c.linebytes for c in bc.CASES.values()})
    jobs = (5, 10, 40, 255, 256, 257, 511, 512, 513, 5120, 0x7fffffff // 5 * 5)
    pairs = [(n, j) for n in lengths for j in jobs]
    got = _launches(exe, 0, 0, pairs)
    assert len(got) == len(pairs)
    for p, g in zip(pairs, got):
        assert g == _parent_launch(*p), p
    assert [g[0] for g in _launches(exe, 0, 0, [(16839, 40), (16840, 40)])] == [1, 0]
    assert [g[1] for g in _launches(exe, 0, 0, [(7281, 40), (7282, 40)])] == [0, 1]
    for p, g in zip(pairs, _launches(exe, 1, 0, pairs)):
        want = _parent_launch(*p)
        row = bc.row_bytes(p[0])
        stride = (65536 * 4 + 4 * p[0] + row + 255) & ~255
        assert g == [0, 0, row, stride, max(1, min(p[1], 256, (1 << 30) // stride)), 0], p
        assert want[0] or g == want
    for cap in (1, 2, 3, 1000):
        for p, g in zip(pairs, _launches(exe, 0, cap, pairs)):
            want = _parent_launch(*p)
            assert g[:4] == want[:4] and g[5] == want[5] and g[4] == min(want[4], cap), (cap, p)


def test_sanitized_program(ref, tmp_path):
    """The stand-alone program under AddressSanitizer and UBSan on the rows where the model's walks leave their arrays if
    they are wrong: rows shorter than the hash, rows of several windows, keys over chunk seams, a slot's owner below 0."""
    _make("SANITIZE=-fsanitize=address,undefined", "SUFFIX=_san")
    san = os.path.join(BUILD, "png_brute_print_san")
    names = ["tiny-2", "tiny-3", "tiny-5", "one-pixel-bw1", "one-pixel-bw8", "chunk-seam-keys-w512", "chunk-1025", "beyond-w256-513",
             "beyond-w2048-2049", "sweep-w1-300", "sweep-w8-300", "sweep-w16384-300"]
    for name in names:
        case = bc.CASES[name]
        size, bits, _, _ = bc.ref_run(ref, case)
        got_size, got_bits = bc.model_run(san, tmp_path, case)
        assert np.array_equal(got_bits, bits) and np.array_equal(got_size, size), name
    pairs = [(1, 5), (7282, 40), (16840, 10), (0x7fffffff, 5)]
    assert _launches(san, 0, 0, pairs) == [_parent_launch(*p) for p in pairs]
