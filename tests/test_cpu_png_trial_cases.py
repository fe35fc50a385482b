"""LodePNG's zlib size on the CPU.  The rules of zopfli_amd/csrc/device/zmx_png_lodeflate.h — the kernels' lanes one after
the other — and of zopfli_amd/csrc/host/png_lodeflate_size.h are run by tests/hostlib/png_lodeflate_print.cc on every
buffer of tests/png_trial_cases.py, at the device's tile length and at short ones (a buffer then spans many tiles and the
links cross them), and must give the length the real LodePNG gave (tests/golden/png_trials.json); the histograms hold the
host's dynamic trees to LodePNG's.  What each case is there to reach is asserted from the bytes alone."""
import os
import subprocess

import numpy as np
import pytest

import png_trial_cases as tc
from zopfli_amd._build import ROOT

HOSTLIB_DIR = os.path.join(ROOT, "tests", "hostlib")
BUILD = os.path.join(ROOT, "tests", "_build")
DEVICE_TILE = 262144
LONG = 140000     # longer buffers run at the device's tile length only


@pytest.fixture(scope="module")
def exe():
    subprocess.check_call(["make", "-s", "-C", HOSTLIB_DIR, "-f", "png_lodeflate.mk"])
    return os.path.join(BUILD, "png_lodeflate_print")


@pytest.fixture(scope="module")
def gold():
    return tc.golden()


def _sizes(exe, tmp_path, names, tile, window=tc.WINDOW, maker=tc.buffer):
    paths = []
    for i, name in enumerate(names):
        paths.append(os.path.join(str(tmp_path), f"b{i}.bin"))
        maker(name).tofile(paths[-1])
    out = subprocess.check_output([exe, "size", str(window), str(tile)] + paths, text=True)
    return [int(v) for v in out.split()]


def test_every_case_has_a_golden(gold):
    assert sorted(gold["buffers"]) == sorted(tc.BUFFER_IDS)
    assert sorted(gold["histograms"]) == sorted(tc.HIST_IDS)
    assert gold["window"] == tc.WINDOW
    for name in tc.IMAGE_IDS:
        for keep in (0, 1):
            assert f"{name}|{keep}|0|-" in gold["images"], name
    for label, (name, _) in tc.PREDEFINED_RUNS.items():
        assert f"{name}|1|0|{label}" in gold["images"] and f"{name}|0|0|{label}" in gold["images"]


@pytest.mark.parametrize("name", tc.BUFFER_IDS)
def test_kernel_rules_give_lodepng_size(exe, gold, tmp_path, name):
    n = len(tc.buffer(name))
    tiles = [DEVICE_TILE] if n > LONG else [DEVICE_TILE, 4096, 1000]
    for tile in tiles:
        assert _sizes(exe, tmp_path, [name], tile) == [gold["buffers"][name]], (name, tile)


def test_mixed_call_equals_singles(exe, gold, tmp_path):
    want = [gold["buffers"][name] for name in tc.MIXED_CALL]
    assert len(tc.MIXED_CALL) == 8
    assert _sizes(exe, tmp_path, tc.MIXED_CALL, DEVICE_TILE) == want
    assert _sizes(exe, tmp_path, tc.MIXED_CALL, 3000) == want


@pytest.mark.parametrize("name", tc.HIST_IDS)
def test_host_trees_give_lodepng_size(exe, gold, tmp_path, name):
    path = os.path.join(str(tmp_path), "h.bin")
    buf = tc.hist_buffer(name)
    assert np.array_equal(np.bincount(buf, minlength=len(tc.HISTOGRAMS[name]))[:len(tc.HISTOGRAMS[name])], tc.HISTOGRAMS[name])
    buf.tofile(path)
    assert int(subprocess.check_output([exe, "huff", path], text=True)) == gold["histograms"][name], name


def _lengths(exe, maxbits, counts):
    return [int(v) for v in subprocess.check_output([exe, "lengths", str(maxbits)] + [str(c) for c in counts], text=True).split()]


def test_code_lengths_respect_their_limits(exe):
    fib = tc.HISTOGRAMS["fibonacci-22"]
    for maxbits, counts in ((15, fib), (7, fib[:12] + [0] * 7), (15, [1] * 286), (7, [1] * 19), (15, [0, 0, 5]), (15, [0] * 30)):
        got = _lengths(exe, maxbits, counts)
        used = [g for g, c in zip(got, counts) if c]
        assert all(1 <= g <= maxbits for g in used), (maxbits, counts, got)
        assert sum(2.0 ** -g for g in got if g) <= 1.0
        if sum(1 for c in counts if c) >= 2:
            assert sum(2.0 ** -g for g in got if g) == 1.0      # a complete code
            assert [g for g, c in zip(got, counts) if not c] == [0] * (len(counts) - len(used))
    # Fibonacci counts want depths beyond the limit: the deepest used length IS the limit
    assert max(_lengths(exe, 15, fib)) == 15 and max(_lengths(exe, 7, fib[:12] + [0] * 7)) == 7
    # LodePNG's two special cases: no symbol, one symbol
    assert _lengths(exe, 15, [0] * 30)[:2] == [1, 1]
    assert _lengths(exe, 15, [0, 0, 5]) == [1, 0, 1] and _lengths(exe, 15, [5, 0, 0]) == [1, 1, 0]


def _longest(a, pos, end, window=tc.WINDOW):
    """(length, distance) of the longest match at pos by plain comparison: the nearest of the longest, within the window
    and not beyond `end`."""
    best = (0, 0)
    for q in range(pos - 1, max(-1, pos - window - 1), -1):
        k = 0
        while pos + k < end and k < 258 and a[q + k] == a[pos + k]:
            k += 1
        if k > best[0]:
            best = (k, pos - q)
    return best


def test_cases_reach_what_they_are_for():
    r = {name: tc.reaches(name) for name in tc.BUFFER_IDS}
    assert [r[k]["n"] for k in ("one-byte", "two-bytes", "three-bytes", "zeros-258")] == [1, 2, 3, 258]
    assert [r[k]["n"] for k in ("noise-8191", "noise-8192", "noise-8193")] == [8191, 8192, 8193]
    assert [r[k]["blocks"] for k in ("block-65535", "block-65536", "block-65537")] == [1, 1, 2]
    assert r["across-ends-131077"]["blocks"] == 3
    assert (r["eight-blocks-600000"]["blocksize"], r["eight-blocks-600000"]["blocks"]) == (75008, 8)
    assert (r["capped-2200000"]["blocksize"], r["capped-2200000"]["blocks"]) == (262144, 9)
    # the far copies: the only match of the repeated bytes is at exactly their distance
    for dist in (8191, 8192, 8193):
        a = tc.buffer(f"copy-at-{dist}")
        assert np.array_equal(a[dist:dist + 64], a[:64]) and len(a) == dist + 64
    a = tc.buffer("across-ends-131077")
    assert not a[65536 - 2500:65536 + 2500].any() and a[65536 - 2501] != 0 or a[65536 + 2500] != 0
    assert np.array_equal(a[-300:], a[20000:20300]) and 131077 - 300 < 131072 < 131077
    # lazy matching: 5 then at most 6; 3 then 7
    a = tc.buffer("lazy-taken")
    p = len(a) - 7
    assert _longest(a, p, len(a))[0] == 5 and _longest(a, p + 1, len(a))[0] <= 6
    a = tc.buffer("lazy-beaten")
    p = len(a) - 9
    assert _longest(a, p, len(a))[0] == 3 and _longest(a, p + 1, len(a))[0] == 7
    # the roll-back in a block's last three positions: 3 at end - 3, nothing of 3 or more after it
    for name, end in (("rollback-at-buffer-end", 3000), ("rollback-at-block-end", 65536)):
        a = tc.buffer(name)
        assert _longest(a, end - 3, end, 300) == (3, 100) and _longest(a, end - 2, end, 300)[0] <= 2, name
        assert _longest(a, end - 4, end, 300)[0] < 3, name
    for dist in (4096, 4097):
        a = tc.buffer(f"len3-at-{dist}")
        assert _longest(a, dist, len(a), dist)[0] == 3 and _longest(a, dist, len(a), dist)[1] == dist
        assert _longest(a, dist, len(a), dist - 1)[0] < 3
    assert _longest(tc.buffer("match-258"), 1, 600) == (258, 1)
    a = tc.buffer("hash0-nonzero")
    assert a[0] != 0 and (int(a[0]) ^ (int(a[1]) << 4) ^ (int(a[2]) << 8)) & 65535 == 0
    # the mixed call: different sizes, more than one block in some
    assert len({r[k]["n"] for k in tc.MIXED_CALL}) == 8 and max(r[k]["blocks"] for k in tc.MIXED_CALL) == 3


def test_images_reach_what_they_are_for(gold):
    g = gold["images"]
    best = {k: v["best"] for k, v in g.items()}
    # a winner of every kind: zero, one of 1 .. 4, minimum sum, entropy, predefined
    assert best["icon-12|1|0|-"] == 0 and best["smooth-rows|1|0|-"] == 1 and best["smooth-columns|1|0|-"] == 2
    assert best["plane|1|0|-"] == 4 and best["halves-noisy|1|0|-"] == 5 and best["halves|1|0|-"] == 6
    assert best["halves|1|0|halves+suited"] == 7 and best["halves|1|0|halves+poor"] == 6
    # ties: the earlier trial wins
    s = g["all-zero|1|0|-"]["sizes"]
    assert s[0] == s[5] == s[6] == min(s) and best["all-zero|1|0|-"] == 0
    s = g["smooth-rows|1|0|-"]["sizes"]
    assert s[1] == s[6] == min(s)
    s = g["plane|1|0|plane+suited"]["sizes"]
    assert s[4] == s[7] == min(s) and best["plane|1|0|plane+suited"] == 4       # predefined ties and loses
    # a column of pixels: Up and Paeth filter alike, as None and Sub do
    img = tc.image("vgrad-w1")
    assert img.shape == (200, 1)
    s = g["vgrad-w1|1|0|-"]["sizes"]
    assert s[0] == s[1] and best["vgrad-w1|1|0|-"] == 2
    # the icon: a palette file below 4096 bytes in every trial, and the second try decides inside the trials
    assert len(np.unique(tc.image("icon-12").reshape(-1, 4), axis=0)) == 12
    assert max(g["icon-12|0|0|-"]["sizes"]) < 4096 and g["icon-12|0|0|-"]["sizes"] != g["icon-12|1|0|-"]["sizes"]
    # --lossy_transparent changes the choice
    assert best["hidden-rows|1|0|-"] != best["hidden-rows|1|1|-"] and best["hidden-rows|0|0|-"] != best["hidden-rows|0|1|-"]
    # without types in the input the predefined trial repeats trial 0
    for k, v in g.items():
        if k.endswith("|-"):
            assert v["sizes"][7] == v["sizes"][0], k
