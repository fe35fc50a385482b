"""zmx_compress_batch: many independent inputs in one pass over the device.  Every output must be the stream that
ZopfliCompress (and the reference) writes for that input alone, whatever else is in the batch; the window floor of
zmx_set_input_segments and the batched checksums of zmx_checksums are checked on their own against the oracle and zlib."""
import gzip
import hashlib
import json
import os
import random
import subprocess
import sys
import threading
import zlib
from collections import defaultdict
from functools import lru_cache

import numpy as np
import pytest

import oracle_lib as ol
from zopfli_amd import Context, ZopfliOptions, api, generate

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")


def _options(numiterations=15, blocksplitting=1, blocksplittingmax=15, verbose=0):
    o = ZopfliOptions()
    o.verbose, o.numiterations, o.blocksplitting, o.blocksplittingmax = verbose, numiterations, blocksplitting, blocksplittingmax
    return o


def _golden_cases(limit):
    out = []
    for name in ("vectors.json", "vectors_extra.json"):
        with open(os.path.join(GOLDEN_DIR, name)) as f:
            out += [c for c in json.load(f) if c["insize"] <= limit]
    return out


def _golden_input(spec):
    if spec["kind"] == "literal":
        from golden.make_golden import LITERALS
        return LITERALS[spec["name"]]
    return generate(spec["cls"], spec["size"], spec.get("seed"))


def _golden_groups():
    groups = defaultdict(list)
    for c in _golden_cases(4000000):
        groups[(c["format"], c["numiterations"], c["blocksplitting"], c["blocksplittingmax"])].append(c)
    return sorted(groups.items())


@pytest.mark.parametrize("key,cases", _golden_groups(), ids=[f"f{k[0]}-n{k[1]}-s{k[2]}-m{k[3]}" for k, _ in _golden_groups()])
def test_golden_batches(gpu_lib, key, cases):
    """Every golden case of at most 4 MB, one batch per (format, numiterations, blocksplitting, blocksplittingmax), in
    order and reversed: each output's length and SHA-256 are the reference's."""
    fmt, n, s, m = key
    datas = [_golden_input(c["input"]) for c in cases]
    for order in (list(range(len(cases))), list(reversed(range(len(cases))))):
        outs = api.compress_batch([datas[i] for i in order], fmt, _options(n, s, m), lib=gpu_lib)
        for i, out in zip(order, outs):
            assert len(out) == cases[i]["outsize"], (cases[i]["input"], order[0])
            assert hashlib.sha256(out).hexdigest() == cases[i]["sha256"], (cases[i]["input"], order[0])


@lru_cache(maxsize=None)
def _leak_files():
    t70 = generate("T", 70000, 11)
    m12 = generate("M", 1200000, 12)
    a = generate("X", 50000, 13)
    b = a[-300:] + generate("X", 40000, 14)          # starts with the previous file's last 300 bytes
    ztail = generate("T", 30000, 15) + bytes(20000)  # ends in a run of zeros ...
    zhead = bytes(5000) + generate("T", 12000, 16)   # ... and the next one starts with zeros
    return [t70, t70, t70, b"", m12, m12, b"x", a, b, b"", ztail, zhead, b"\0"]


@lru_cache(maxsize=None)
def _ref_out(data, fmt, bs):
    return ol.ref_compress(data, fmt, 15, bs, 15)


@pytest.mark.parametrize("bs", [0, 1])
@pytest.mark.parametrize("fmt", [api.FORMAT_GZIP, api.FORMAT_ZLIB, api.FORMAT_DEFLATE])
def test_no_leakage_across_inputs(gpu_lib, fmt, bs):
    """Inputs that would find matches in the input before them (the same file again, a shared 300-byte seam, a run of
    zeros across the boundary, empty and 1-byte files between them): each output equals the single call's and the
    reference's for that input alone."""
    files = _leak_files()
    opts = _options(15, bs, 15)
    outs = api.compress_batch(files, fmt, opts, lib=gpu_lib)
    assert len(outs) == len(files)
    single = {}
    for i, (f, out) in enumerate(zip(files, outs)):
        if f not in single:
            single[f] = api.compress(f, fmt, opts, lib=gpu_lib)
        assert out == single[f], (i, len(f))
        assert out == _ref_out(f, fmt, bs), (i, len(f))


def _assert_tables_match(ctx, t, b, data, rel_s, rel_e, off):
    o = ol.OracleTable(data, rel_s, rel_e)
    try:
        for rel in range(rel_s, rel_e):
            gl, gd, gsub = t.find_longest_match(b, off + rel)
            ol_, od, osub = o.find_longest_match(rel)
            assert (gl, gd) == (ol_, od) or (gl < 3 and ol_ < 3), (rel_s, rel)
            if ol_ >= 3:
                assert np.array_equal(gsub[3:ol_ + 1], osub[3:ol_ + 1]), (rel_s, rel)
        for g, r in zip(t.hash_links(b), o.hash_links()):
            assert np.array_equal(g, r), rel_s
        nsym, _ = t.greedy(0)
        gll, gdd = t.store(b, 0, nsym[b])
        oll, odd = o.greedy()
        assert np.array_equal(gll, oll) and np.array_equal(gdd, odd), rel_s
    finally:
        o.close()


def test_tables_with_segments_match_oracle(gpu_lib):
    """Three inputs end to end with their segments declared: tables of blocks of the middle one (at its first byte,
    10 000 and 40 000 bytes in) are the oracle's for that input alone — every match record, the hash links, the
    greedy store.  A block across two segments is refused; after a plain set_input the window is the whole input's."""
    first = generate("T", 45000, 21)                        # longer than the window
    middle = first[-20000:] + generate("T", 90000, 22)      # tempting matches into `first` without the floor
    last = middle[:30000] + generate("X", 10000, 23)
    cat = first + middle + last
    off = len(first)
    ctx = Context(0, gpu_lib)
    try:
        ctx.set_input(cat)
        ctx.set_input_segments([0, len(first), len(first) + len(middle)])
        for rel_s, rel_e in ((0, 30000), (10000, 45000), (40000, len(middle))):
            t = ctx.build_tables([(off + rel_s, off + rel_e)])
            try:
                _assert_tables_match(ctx, t, 0, middle, rel_s, rel_e, off)
            finally:
                t.free()
        with pytest.raises(RuntimeError, match="segments"):
            ctx.build_tables([(off - 100, off + 100)])
        assert gpu_lib.zmx_last_error_class() == 3   # ZMX_ERR_REFUSED
        with pytest.raises(RuntimeError):
            ctx.set_input_segments([5, 10])             # starts[0] must be 0
        ctx.set_input(cat)                              # one segment again
        t = ctx.build_tables([(off + 10000, off + 45000)])
        try:
            _assert_tables_match(ctx, t, 0, cat, off + 10000, off + 45000, 0)
        finally:
            t.free()
    finally:
        ctx.close()


def test_batched_checksums_match_zlib(gpu_ctx):
    """zmx_checksums over 10 000+ ranges in one call against zlib: empty and 1-byte ranges, ranges ending on the
    kernel's 4 B, 1 KiB and 256 KiB boundaries, random ranges and one of about 20 MB."""
    data = generate("X", 21000000, 31)
    n = len(data)
    rng = random.Random(5)
    marks = [0, 1, 2, 3, 4, 5, 1023, 1024, 1025, 2048, 262143, 262144, 262145, 524288, 524289]
    ranges = [(a, b) for a in marks for b in marks if a <= b]
    ranges += [(7, 7), (n, n), (n - 1, n), (0, n), (123, 20000123)]
    for _ in range(10000):
        a = rng.randrange(n)
        b = min(n, a + rng.choice([0, 1, 3, 4, 5, rng.randrange(70000), 262144 - rng.randrange(8), 1024 * rng.randrange(1, 300)]))
        ranges.append((a, b))
    gpu_ctx.set_input(data)
    mv = memoryview(data)
    crc = gpu_ctx.checksums(api.CRC32, ranges)
    adl = gpu_ctx.checksums(api.ADLER32, ranges)
    for (a, b), c, d in zip(ranges, crc, adl):
        assert c == zlib.crc32(mv[a:b]), (a, b)
        assert d == zlib.adler32(mv[a:b]), (a, b)
    assert gpu_ctx.checksums(api.CRC32, []) == []
    with pytest.raises(RuntimeError):
        gpu_ctx.checksums(api.CRC32, [(0, n + 1)])
    with pytest.raises(RuntimeError):
        gpu_ctx.checksums(7, [(0, 1)])


def _many_files():
    rng = random.Random(2024)
    out = []
    for i in range(3000):
        out.append(generate(rng.choice("TXRZBPM"), rng.randrange(20001), i + 1))
    return out


_MANY_SCRIPT = """
import hashlib, sys
sys.path[:0] = [{root!r}, {tests!r}]
from zopfli_amd import api
from test_gpu_batch import _many_files
outs = api.compress_batch(_many_files(), api.FORMAT_GZIP)
print(hashlib.sha256(b"".join(hashlib.sha256(o).digest() for o in outs)).hexdigest())
"""


def test_many_small_files_over_several_contexts(gpu_lib):
    """3 000 files of 0 - 20 000 bytes of mixed classes, gzip, default options: every output decompresses to its input,
    50 sampled outputs are the reference's, and the batch dealt over two device entries (ZOPFLI_AMD_DEVICES=0,0: more
    contexts) in a fresh process gives the same bytes."""
    files = _many_files()
    outs = api.compress_batch(files, api.FORMAT_GZIP, lib=gpu_lib)
    assert len(outs) == len(files)
    for f, o in zip(files, outs):
        assert gzip.decompress(o) == f
    for i in random.Random(9).sample(range(len(files)), 50):
        assert outs[i] == ol.ref_compress(files[i], 0), i
    here = hashlib.sha256(b"".join(hashlib.sha256(o).digest() for o in outs)).hexdigest()
    env = dict(os.environ, ZOPFLI_AMD_DEVICES="0,0")
    r = subprocess.run([sys.executable, "-c", _MANY_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, "tests"))],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split()[-1] == here


def test_concurrent_batches_and_single_calls(gpu_lib):
    """Two threads call compress_batch while a third calls ZopfliCompress: every output is the single call's."""
    rng = random.Random(77)
    sets = [[generate(rng.choice("TXMZ"), rng.randrange(1, 150000), 1000 * k + i) for i in range(40)] for k in range(3)]
    want = [[api.compress(f, lib=gpu_lib) for f in s] for s in sets]
    got = [None, None, None]
    errors = []

    def batch(k):
        try:
            got[k] = api.compress_batch(sets[k], lib=gpu_lib)
        except Exception as e:  # noqa: BLE001 - reported below
            errors.append(e)

    def single():
        try:
            got[2] = [api.compress(f, lib=gpu_lib) for f in sets[2]]
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=batch, args=(0,)), threading.Thread(target=batch, args=(1,)),
               threading.Thread(target=single)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k in range(3):
        assert got[k] == want[k], k


def test_edges(gpu_lib):
    """n = 0 returns 0 with nothing written; an unknown format is refused with a message."""
    assert api.compress_batch([], lib=gpu_lib) == []
    import ctypes
    fn = gpu_lib.zmx_compress_batch
    opts = ZopfliOptions()
    assert fn(ctypes.byref(opts), 0, 0, None, None, None, None) == 0
    with pytest.raises(RuntimeError, match="ZopfliFormat"):
        api.compress_batch([b"abc"], 7, lib=gpu_lib)
    assert gpu_lib.zmx_last_error_class() == 3   # ZMX_ERR_REFUSED


_VERBOSE_SCRIPT = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
from zopfli_amd import ZopfliOptions, api, generate
files = [generate("T", 30000, 1), b"", generate("M", 70000, 2)]
o = ZopfliOptions()
o.verbose = 1
if sys.argv[1] == "batch":
    api.compress_batch(files, {fmt}, o)
else:
    for f in files:
        api.compress(f, {fmt}, o)
"""


@pytest.mark.parametrize("fmt", [api.FORMAT_GZIP, api.FORMAT_DEFLATE])
def test_verbose_lines_in_input_order(fmt):
    """verbose = 1: the batch prints what the three single calls print, in input order."""
    script = _VERBOSE_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, "tests"), fmt=fmt)
    err = {}
    for mode in ("batch", "single"):
        r = subprocess.run([sys.executable, "-c", script, mode], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        err[mode] = r.stderr
    assert "Original Size" in err["single"]
    assert err["batch"] == err["single"]
