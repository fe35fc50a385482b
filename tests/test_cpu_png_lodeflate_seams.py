"""The k_png_lo_* kernels' rules (zopfli_amd/csrc/device/zmx_png_lodeflate.h) word by word, on the CPU:
tests/hostlib/png_lodeflate_print.cc runs the lanes one after the other and hands out the per-position arrays HC, ZC, LD
and every deflate block's 316 symbol counts and extra bits.  On the cases of tests/png_lodeflate_seam_cases.py they must
not depend on the tile length, and the counts and the size must be the real LodePNG's (encodeLZ77 per block behind
oracle/_ref/libpng_lodeflate_ref.so) at every window the case runs at: 256 .. 32768, so the chain cap of W / 8 and the
lazy limit of 64 below 8192 are tied to LodePNG too.  The program also runs under AddressSanitizer and UBSan, and every
case's reason for being there is asserted from its bytes."""
import os
import subprocess

import numpy as np
import pytest

import png_lodeflate_seam_cases as sc
from zopfli_amd._build import PNG_LODEFLATE_REF, ROOT

HOSTLIB_DIR = os.path.join(ROOT, "tests", "hostlib")
BUILD = os.path.join(ROOT, "tests", "_build")
ARRAYS = ("HC", "ZC", "LD")


@pytest.fixture(scope="module")
def exe():
    subprocess.check_call(["make", "-s", "-C", HOSTLIB_DIR, "-f", "png_lodeflate.mk"])
    return os.path.join(BUILD, "png_lodeflate_print")


@pytest.fixture(scope="module")
def ref():
    if not os.path.exists(PNG_LODEFLATE_REF):
        pytest.skip("oracle/_ref/libpng_lodeflate_ref.so not built (the reference's tree is not at hand)")
    return sc.ref_library(PNG_LODEFLATE_REF)


@pytest.mark.parametrize("name", sc.CASE_IDS)
def test_cases_reach_what_they_are_for(name):
    sc.CASES[name].check()


def test_the_lists_are_used():
    runs = [r for c in sc.CASES.values() for r in c.runs]
    assert {w for w, _ in runs} == set(sc.WINDOWS) and set(sc.TILES) <= {t for _, t in runs}
    mixed = [sc.CASES[name].runs[0] for name in sc.MIXTURES]
    assert len(mixed) == 24 and {w for w, _ in mixed} == set(sc.WINDOWS) and {t for _, t in mixed} == set(sc.TILES)
    # every outcome of the lazy match at the refill, and the held match on either side of it
    names = [n for n in sc.CASE_IDS if n.startswith("parse-refill-")]
    assert {n.split("-", 3)[3] for n in names} == set(sc.REFILL_OUTCOMES) and {int(n.split("-")[2]) for n in names} == set(sc.REFILL_X)
    assert {"parse-refill-2047-beaten", "parse-refill-2047-taken", "parse-refill-2047-jump-258", "parse-refill-2048-taken"} <= set(names)


@pytest.mark.parametrize("name", sc.CASE_IDS)
def test_arrays_do_not_depend_on_the_tile_length(exe, tmp_path, name):
    case = sc.CASES[name]
    bufs = case.bufs()
    assert max(len(b) for b in bufs) <= sc.DEVICE_TILE
    for window in case.windows:
        whole = sc.cpu_run(exe, tmp_path, bufs, window, 0)       # one tile for the whole buffer
        for tile in sorted({t for w, t in case.runs if t and w == window}):
            got = sc.cpu_run(exe, tmp_path, bufs, window, tile)
            for k, what in enumerate(ARRAYS):
                assert np.array_equal(got[1 + k], whole[1 + k]), (window, tile, sc.differences(what, got[1 + k], whole[1 + k], bufs, tile))
            assert np.array_equal(got[4], whole[4]), (window, tile, "counts")
            assert got[0] == whole[0], (window, tile)


@pytest.mark.parametrize("name", sc.CASE_IDS)
def test_hashes_zero_runs_and_links_are_the_models(exe, tmp_path, name):
    """HC and ZC against numpy's statement of them (sc.model_words): the hash, the zero run and the slot every position's
    insertion writes, whichever of the three kernels made it."""
    case = sc.CASES[name]
    bufs = case.bufs()
    at, _ = sc.plan_offsets(bufs)
    for window, tile in case.runs:
        _, hc, zc, _, _ = sc.cpu_run(exe, tmp_path, bufs, window, tile)
        for i, b in enumerate(bufs):
            want_hc, want_zc = sc.model_words(b, window)
            for what, got, want in (("HC", hc, want_hc), ("ZC", zc, want_zc)):
                got = got[at[i]:at[i + 1]]
                assert np.array_equal(got, want), (window, tile, "buffer", i, sc.differences(what, got, want, [b], tile))


def test_every_buffer_of_a_call_as_if_alone(exe, tmp_path):
    """[A, A, B, A]: every buffer's slice of the call's arrays is what the buffer gives in a call of its own."""
    case = sc.CASES["same-bytes-twice"]
    bufs = case.bufs()
    at, blk = sc.plan_offsets(bufs)
    for window, tile in case.runs:
        sizes, hc, zc, ld, counts = sc.cpu_run(exe, tmp_path, bufs, window, tile)
        for i, b in enumerate(bufs):
            one = sc.cpu_run(exe, tmp_path, [b], window, tile)
            assert [sizes[i]] == one[0], (window, tile, i)
            for what, got, want in zip(ARRAYS, (hc, zc, ld), one[1:4]):
                got = got[at[i]:at[i + 1]]
                assert np.array_equal(got, want), (window, tile, "buffer", i, sc.differences(what, got, want, [b], tile))
            assert np.array_equal(counts[blk[i]:blk[i + 1]], one[4]), (window, tile, i, "counts")


@pytest.mark.parametrize("name", sc.CASE_IDS)
def test_counts_and_size_are_lodepngs(exe, ref, tmp_path, name):
    case = sc.CASES[name]
    bufs = case.bufs()
    done = set()
    for window, tile in case.runs:
        if window in done:
            continue
        done.add(window)
        want_sizes, want_counts = sc.ref_run(ref, bufs, window)
        sizes, _, _, _, counts = sc.cpu_run(exe, tmp_path, bufs, window, tile)
        bad = np.argwhere(counts != want_counts)[:5]
        assert not len(bad), (window, tile, [(int(b), int(s), int(counts[b, s]), int(want_counts[b, s])) for b, s in bad])
        assert sizes == want_sizes, (window, tile)


def test_sanitized_program(tmp_path):
    """The `arrays` mode as a stand-alone program under AddressSanitizer and UBSan on the walks that leave their tile: a KEEP
    walk below position 0, an ASK walk in front of the buffer's first table, a read behind a tile's last live lane."""
    subprocess.check_call(["make", "-s", "-C", HOSTLIB_DIR, "-f", "png_lodeflate.mk", "SANITIZE=-fsanitize=address,undefined", "SUFFIX=_san"])
    san = os.path.join(BUILD, "png_lodeflate_print_san")
    plain = os.path.join(BUILD, "png_lodeflate_print")
    subprocess.check_call(["make", "-s", "-C", HOSTLIB_DIR, "-f", "png_lodeflate.mk"])
    names = [n for n in sc.CASE_IDS if n.startswith("never-seen-")] + ["zero-runs-over-seams", "same-bytes-twice"]
    assert len(names) == 7
    for name in names:
        case = sc.CASES[name]
        for window, tile in case.runs:
            got = sc.cpu_run(san, tmp_path, case.bufs(), window, tile)
            want = sc.cpu_run(plain, tmp_path, case.bufs(), window, tile)
            assert got[0] == want[0] and all(np.array_equal(g, w) for g, w in zip(got[1:], want[1:])), (name, window, tile)
