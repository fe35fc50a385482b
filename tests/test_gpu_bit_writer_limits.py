"""The device bit writer (zmx_encode_blocks: k_enc_len, k_enc_scan, k_enc_emit, zmx_encode.h) away from the fixed tree:
symbols of 48 bits (the third LDS word of k_enc_emit), a tile whose bits fill its whole buffer, a 15-bit end symbol
across a word, stores of exactly k * 2048 symbols (the last tile holds the end symbol alone), more than 64 tiles in a job
(k_enc_scan's loop), one code table per job.  The stores are steered ones (steer_cases.py), each first held equal to the
oracle's so that a parse fault is not reported as a writer fault; the reference is the bit-by-bit Python writer of
test_gpu_parity.py, applied tile by tile (steer_cases.write_symbols; test_cpu_steer_cases.py holds that to the plain
writer).  The code tables are arbitrary (bits, length << 16) arrays: zmx_encode_blocks asks for no prefix code and the
Python writer does not care.  Byte equality, no tolerance."""
import numpy as np
import pytest

import steer_cases as sc
from test_gpu_parity import _py_symbol_bits

pytestmark = pytest.mark.gpu


def _steered_tables(gpu_ctx, name):
    """Tables with the steered store `name` in slot 1 of every block, equal to the oracle's: (Tables, case, nsym)."""
    c = sc.steered(name)
    gpu_ctx.set_input(c["data"])
    t = gpu_ctx.build_tables(c["blocks"])
    try:
        nb = len(c["blocks"])
        t.greedy(0)
        nsym, hist = t.squeeze_run(c["cost"], c["mincost"], np.ones(nb, dtype=np.int32))
        sc.assert_run_equals_oracle(t, c["blocks"], 1, nsym, hist, c["runs"], name)
    except BaseException:
        t.free()
        raise
    return t, c, nsym


def _check(t, jobs):
    """jobs = [(block, slot, litlens, dists, codes, bit_start)]: one zmx_encode_blocks call, every output equal to the
    Python writer's bytes and the 8 bytes of slack behind it untouched."""
    want, call = [], []
    for block, slot, ll, dd, codes, start in jobs:
        by, nb = sc.write_symbols(_py_symbol_bits, ll, dd, codes, start)
        assert nb == int(sc.symbol_bits(ll, dd, codes).sum()) + (int(codes[256]) >> 16)
        want.append(by)
        call.append((block, slot, len(ll), start, nb))
    got = t.encode_blocks(call, np.stack([j[4] for j in jobs]), slack=True)
    for i, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w) + 8
        if g[:len(w)] != w:
            first = next(k for k in range(len(w)) if g[k] != w[k])
            raise AssertionError(f"job {i} (block {call[i][0]}, {call[i][2]} symbols, bit_start {call[i][3]}): byte {first} of "
                                 f"{len(w)} is {g[first]:#x}, the Python writer has {w[first]:#x}")
        assert g[len(w):] == bytes(8), f"job {i}: slack behind the output written"
    return call


def test_full_48bit_tile(gpu_ctx):
    """2068 symbols of 48 bits each: the first tile's 98304 bits are all of its LDS buffer, every symbol at an odd word
    offset needs the third word.  As 33 jobs of one call that name the same block and slot, at bit_start 0 .. 31 and
    4100; then with a mixed and a sparse table; and a wrong nbits (one less, one more) is refused."""
    t, c, nsym = _steered_tables(gpu_ctx, "tile48")
    try:
        la, ll, dd = c["runs"][0]
        codes = sc.codes_15bit(11)
        bits = sc.symbol_bits(ll, dd, codes)
        assert sc.longest_run_of(bits, 48) >= 2068 and sc.tile_starts(bits)[1][0] == sc.ENC_TILE * 48
        call = _check(t, [(0, 1, ll, dd, codes, start) for start in list(range(32)) + [4100]])
        _check(t, [(0, 1, ll, dd, sc.codes_mixed(12), 7), (0, 1, ll, dd, sc.codes_sparse(ll, dd, 13), 0),
                   (0, 1, ll, dd, sc.codes_15bit(14), 63)])
        for off in (-1, 1):
            bad = list(call[3])
            bad[4] += off
            with pytest.raises(RuntimeError, match="different number of bits"):
                t.encode_blocks([tuple(bad)], codes)
    finally:
        t.free()


def test_literal_mixed_tile(gpu_ctx):
    """The 48-bit store with literals in between: by the writer's own bookkeeping a symbol with sh + n > 64 occurs at every
    shift sh = 17 .. 31 of its tile's buffer, and prefixes of the store put a 15-bit end symbol across a word at every
    shift 18 .. 31 (a job may take any prefix of a store)."""
    t, c, nsym = _steered_tables(gpu_ctx, "tile48_mixed")
    try:
        la, ll, dd = c["runs"][0]
        codes = sc.codes_15bit(21)
        bits = sc.symbol_bits(ll, dd, codes)
        assert sc.three_word_shifts(bits) >= set(range(17, 32))
        ends = sc.end_symbol_prefixes(bits)
        assert set(ends) == set(range(18, 32))
        jobs = [(0, 1, ll, dd, codes, start) for start in (0, 5, 31)]
        jobs += [(0, 1, ll[:n], dd[:n], codes, sh % 7) for sh, n in sorted(ends.items())]
        jobs += [(0, 1, ll, dd, sc.codes_mixed(22), 13), (0, 1, ll, dd, sc.codes_sparse(ll, dd, 23), 2)]
        _check(t, jobs)
    finally:
        t.free()


def test_all_literal_stores(gpu_ctx):
    """Stores of exactly 2047, 2048, 2049 and 4096 symbols (at a tile multiple the last tile holds the end symbol alone)
    and of 64 * 2048 + 1 symbols (65 tiles: k_enc_scan's loop goes round twice), under 15-bit codes, a mixed table and a
    sparse one, at ragged bit offsets."""
    t, c, nsym = _steered_tables(gpu_ctx, "literals")
    try:
        assert [int(x) for x in nsym] == [2047, 2048, 2049, 4096, 64 * sc.ENC_TILE + 1]
        jobs = []
        for b, (la, ll, dd) in enumerate(c["runs"]):
            jobs.append((b, 1, ll, dd, sc.codes_15bit(30 + b), (0, 3, 77, 31, 64)[b]))
            jobs.append((b, 1, ll, dd, sc.codes_mixed(40 + b), (17, 0, 1, 4099, 5)[b]))
            jobs.append((b, 1, ll, dd, sc.codes_sparse(ll, dd, 50 + b), (8, 9, 0, 2, 30)[b]))
        _check(t, jobs)
    finally:
        t.free()


def test_one_code_table_per_job(gpu_ctx):
    """45 jobs of ragged sizes in one call — prefixes of greedy stores of mixed data, from no symbol at all to 20000 —
    each with a code table of its own (15-bit, mixed, sparse by turns): every output is exact and its slack stays zero."""
    from zopfli_amd import generate
    data = generate("M", 200000)
    blocks = [(0, 2500), (2500, 90000), (90000, 200000)]
    gpu_ctx.set_input(data)
    t = gpu_ctx.build_tables(blocks)
    try:
        nsym, _ = t.greedy(0)
        stores = [t.store(b, 0, nsym[b]) for b in range(len(blocks))]
        for b, (s, e) in enumerate(blocks):
            oll, odd = sc.oracle_tables(data, blocks)[b].greedy()
            assert np.array_equal(stores[b][0], oll) and np.array_equal(stores[b][1], odd)
        sizes = [0, 1, 2, 7, 63, 64, 65, 255, 256, 257, 300, 511, 777, 1023, 1024, 2000, 2046, 2047, 2048, 2049, 2050, 3000,
                 4095, 4096, 4097, 5000, 6143, 6144, 6145, 7001, 8191, 8192, 8193, 9999, 10240, 12287, 12288, 12289, 15000,
                 16383, 16384, 16385, 18000, 19999, 20000]
        assert len(sizes) >= 40
        jobs = []
        for i, n in enumerate(sizes):
            b = 1 + (i & 1) if n > int(nsym[0]) or i % 3 else 0
            n = min(n, int(nsym[b]))
            ll, dd = stores[b][0][:n], stores[b][1][:n]
            codes = (sc.codes_15bit(100 + i), sc.codes_mixed(100 + i), sc.codes_sparse(ll, dd, 100 + i))[i % 3]
            jobs.append((b, 0, ll, dd, codes, (i * 37) % 101))
        assert len({j[4].tobytes() for j in jobs}) == len(jobs)
        _check(t, jobs)
    finally:
        t.free()
