"""zmx_compress_device_batch: many inputs that lie in device memory in one call.  Every output must be what
zmx_compress_batch gives for the same bytes on the host and what ZopfliCompress gives for that input alone, whatever
the other inputs, their addresses and the contexts the batch is dealt over.  Device buffers come from torch."""
import ctypes
import hashlib
import json
import os
import random
import re
import subprocess
import sys
import threading
from collections import defaultdict
from functools import lru_cache

import numpy as np
import pytest
import torch

from zopfli_amd import ZopfliOptions, api, generate

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "vectors.json")
ZMX_ERR_REFUSED = 3
FORMATS = [api.FORMAT_GZIP, api.FORMAT_ZLIB, api.FORMAT_DEFLATE]


def _dev(data):
    if len(data) == 0:
        return torch.empty(0, dtype=torch.uint8, device="cuda")
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


@lru_cache(maxsize=None)
def _leak_files():
    t70 = generate("T", 70000, 11)
    m12 = generate("M", 1200000, 12)                 # two master blocks
    a = generate("X", 50000, 13)
    b = a[-300:] + generate("X", 40000, 14)          # begins with the last 300 bytes of the input before it
    ztail = generate("T", 30000, 15) + bytes(20000)  # ends in zeros ...
    zhead = bytes(5000) + generate("T", 12000, 16)   # ... and the next one starts with zeros
    return [t70, t70, t70, b"", m12, b"x", a, b, b"", ztail, zhead, b"\0"]


@lru_cache(maxsize=None)
def _leak_want(fmt, bs):
    """The host batch's outputs and the single calls', computed once."""
    lib = api.library()
    files = _leak_files()
    opt = ZopfliOptions(5, bs)
    batch = api.compress_batch(files, fmt, opt, lib=lib)
    single = {}
    for f in files:
        if f not in single:
            single[f] = api.compress(f, fmt, opt, lib=lib)
    assert batch == [single[f] for f in files]
    return batch


@pytest.mark.parametrize("bs", [0, 1])
@pytest.mark.parametrize("fmt", FORMATS)
def test_no_leakage_across_inputs(gpu_lib, fmt, bs):
    """Inputs that would find matches in the input before them: each output is the host batch's and the single call's."""
    tensors = [_dev(f) for f in _leak_files()]
    outs = api.compress_device_batch(tensors, fmt, ZopfliOptions(5, bs), lib=gpu_lib)
    assert outs == _leak_want(fmt, bs)


@pytest.mark.parametrize("bs", [0, 1])
@pytest.mark.parametrize("fmt", FORMATS)
def test_adjacent_slices_at_odd_offsets(gpu_lib, fmt, bs):
    """The same inputs as adjacent slices of ONE allocation that starts at an odd offset: neighbours in memory are still
    independent inputs (the window floor comes from the list, not from the addresses), (pointer, nbytes) pairs."""
    files = _leak_files()
    whole = torch.full((64 + 3 + sum(len(f) for f in files) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    pairs, at = [], 64 + 3
    for f in files:
        if f:
            whole[at:at + len(f)].copy_(_dev(f))
        pairs.append((whole.data_ptr() + at, len(f)))
        at += len(f)
    assert pairs[0][0] % 2 == 1
    torch.cuda.synchronize()
    before = whole.cpu().numpy().copy()
    outs = api.compress_device_batch(pairs, fmt, ZopfliOptions(5, bs), lib=gpu_lib)
    assert outs == _leak_want(fmt, bs)
    assert np.array_equal(whole.cpu().numpy(), before)


def _golden_groups():
    with open(GOLDEN) as f:
        cases = [c for c in json.load(f) if c["insize"] <= 1200000]
    groups = defaultdict(list)
    for c in cases:
        groups[(c["format"], c["numiterations"], c["blocksplitting"], c["blocksplittingmax"])].append(c)
    return sorted(groups.items())


def _golden_input(spec):
    if spec["kind"] == "literal":
        from golden.make_golden import LITERALS
        return LITERALS[spec["name"]]
    return generate(spec["cls"], spec["size"], spec.get("seed"))


@pytest.mark.parametrize("key,cases", _golden_groups(), ids=[f"f{k[0]}-n{k[1]}-s{k[2]}-m{k[3]}" for k, _ in _golden_groups()])
def test_golden_batches(gpu_lib, key, cases):
    """The golden cases of at most 1 200 000 bytes, one batch per option group: the reference's length and SHA-256."""
    fmt, n, s, m = key
    tensors = [_dev(_golden_input(c["input"])) for c in cases]
    outs = api.compress_device_batch(tensors, fmt, ZopfliOptions(n, s, m), lib=gpu_lib)
    for c, out in zip(cases, outs):
        assert len(out) == c["outsize"], c["input"]
        assert hashlib.sha256(out).hexdigest() == c["sha256"], c["input"]


def test_input_traffic(gpu_lib):
    """Nothing of text inputs visits the host: [0] = 0 host to device, [2] = 0 device to host, [1] at least the inputs
    (the gather and the shards' copies).  A random input brings down its stored blocks' bytes, no more."""
    opt = ZopfliOptions(5)
    texts = [generate("T", 70000, 1), generate("T", 30000, 2) + bytes(20000), generate("X", 50000, 3)]
    total = sum(len(t) for t in texts)
    api.compress_device_batch([_dev(t) for t in texts], options=opt, lib=gpu_lib)
    t = api.last_input_traffic(gpu_lib)
    assert t[0] == 0 and t[2] == 0 and t[1] >= total, t
    noise = np.random.default_rng(1).integers(0, 256, 100000, dtype=np.uint8).tobytes()
    files = texts[:2] + [noise] + texts[2:]
    outs = api.compress_device_batch([_dev(f) for f in files], options=opt, lib=gpu_lib)
    t = api.last_input_traffic(gpu_lib)
    assert t[0] == 0 and 0 < t[2] <= len(noise), t
    assert outs == api.compress_batch(files, options=opt, lib=gpu_lib)


def _forty_files():
    rng = random.Random(41)
    return [generate(rng.choice("TXMZ"), rng.randrange(30000, 150001), 100 + i) for i in range(40)]


def _dealing_files():
    """Z-class files (long runs: several times the cost of text) among text files."""
    return [generate("Z" if i % 5 == 2 else "T", 60000 + 9000 * (i % 7), 300 + i) for i in range(40)]


_CHILD = """
import hashlib, sys
sys.path[:0] = [{root!r}, {tests!r}]
import torch
from zopfli_amd import ZopfliOptions, api
import test_gpu_device_batch as t
files = getattr(t, sys.argv[2])()
opt = ZopfliOptions(5, 1)
if sys.argv[1] == "device":
    tensors = [t._dev(f) for f in files]
    torch.cuda.synchronize()
    outs = api.compress_device_batch(tensors, options=opt)
else:
    outs = api.compress_batch(files, options=opt)
print(hashlib.sha256(b"".join(hashlib.sha256(o).digest() for o in outs)).hexdigest())
"""


def _child(mode, files, **env):
    script = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", script, mode, files], env=dict(os.environ, **env), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.split()[-1], r.stderr


def test_several_contexts(gpu_lib):
    """40 inputs of 30 - 150 KB with block splitting: the host batch's bytes, and the same bytes from a fresh process
    that deals the batch over two device entries (ZOPFLI_AMD_DEVICES=0,0: more contexts)."""
    files = _forty_files()
    opt = ZopfliOptions(5, 1)
    outs = api.compress_device_batch([_dev(f) for f in files], options=opt, lib=gpu_lib)
    assert outs == api.compress_batch(files, options=opt, lib=gpu_lib)
    here = hashlib.sha256(b"".join(hashlib.sha256(o).digest() for o in outs)).hexdigest()
    there, _ = _child("device", "_forty_files", ZOPFLI_AMD_DEVICES="0,0")
    assert there == here


def test_same_dealing_as_the_host_batch():
    """The counts taken on the staging buffer give the dealing the host batch computes from its bytes: the
    `shard k (N parts)` lines of ZOPFLI_AMD_TRACE_CALL=1 are the same in both, on Z-class files among text."""
    shards = {}
    digest = {}
    for mode in ("device", "host"):
        digest[mode], err = _child(mode, "_dealing_files", ZOPFLI_AMD_TRACE_CALL="1")
        shards[mode] = sorted((int(k), int(n)) for k, n in re.findall(r"shard (\d+) \((\d+) parts\)", err))
    print("shards (index, parts):", shards["host"])
    assert len(shards["host"]) >= 2, "the batch was not dealt: the test shows nothing"
    assert shards["device"] == shards["host"]
    assert digest["device"] == digest["host"]


def _raw_batch(lib, ptrs, sizes, fmt=api.FORMAT_GZIP):
    """zmx_compress_device_batch on output arrays that already hold something: (return code, what they hold after)."""
    n = len(ptrs)
    fn = lib.zmx_compress_device_batch
    fn.argtypes = [ctypes.POINTER(ZopfliOptions), ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p),
                   ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]
    fn.restype = ctypes.c_int
    libc = ctypes.CDLL(None)
    libc.malloc.restype = ctypes.c_void_p
    libc.malloc.argtypes = [ctypes.c_size_t]
    libc.free.argtypes = [ctypes.c_void_p]
    addrs = [libc.malloc(16) for _ in range(n)]
    for a in addrs:
        ctypes.memmove(a, b"0123456789abcdef", 16)
    outs = (ctypes.c_void_p * n)(*addrs)
    outsizes = (ctypes.c_size_t * n)(*([3] * n))
    opt = ZopfliOptions(5)
    rc = fn(ctypes.byref(opt), fmt, n, (ctypes.c_void_p * n)(*ptrs), (ctypes.c_size_t * n)(*sizes), outs, outsizes)
    after = [(outs[i], outsizes[i], ctypes.string_at(outs[i], 16) if outs[i] == addrs[i] else None) for i in range(n)]
    for i in range(n):
        libc.free(outs[i])
    return rc, after, [(a, 3, b"0123456789abcdef") for a in addrs]


def test_refusals(gpu_lib):
    """A host pointer as input 3 of 5: -1 with ZMX_ERR_REFUSED, every out[i] and outsize[i] as before, and the next
    valid call is right.  n = 0 with null arrays is 0; a bad format is refused."""
    files = [generate("T", 20000 + 1000 * i, 50 + i) for i in range(5)]
    tensors = [_dev(f) for f in files]
    torch.cuda.synchronize()
    on_host = np.frombuffer(files[2], dtype=np.uint8).copy()
    ptrs = [t.data_ptr() for t in tensors]
    sizes = [len(f) for f in files]
    for bad in (on_host.ctypes.data, 0):
        rc, after, before = _raw_batch(gpu_lib, ptrs[:2] + [bad] + ptrs[3:], sizes)
        assert rc == -1
        assert gpu_lib.zmx_last_error_class() == ZMX_ERR_REFUSED, gpu_lib.zmx_last_error()
        assert after == before
        with pytest.raises(RuntimeError):
            api.compress_device_batch(list(zip(ptrs[:2] + [bad] + ptrs[3:], sizes)), lib=gpu_lib)
        opt = ZopfliOptions(5)
        assert api.compress_device_batch(tensors, options=opt, lib=gpu_lib) == api.compress_batch(files, options=opt, lib=gpu_lib)
    rc, after, before = _raw_batch(gpu_lib, ptrs, sizes, fmt=7)
    assert rc == -1 and after == before
    assert gpu_lib.zmx_last_error_class() == ZMX_ERR_REFUSED
    with pytest.raises(RuntimeError, match="ZopfliFormat"):
        api.compress_device_batch(tensors, 7, lib=gpu_lib)
    with pytest.raises(ValueError):
        api.compress_device_batch([tensors[0], tensors[1][::2]], lib=gpu_lib)
    assert api.compress_device_batch([], lib=gpu_lib) == []
    fn = gpu_lib.zmx_compress_device_batch
    opts = ZopfliOptions()
    assert fn(ctypes.byref(opts), 0, 0, None, None, None, None) == 0


def test_concurrent_batches_and_reuse(gpu_lib):
    """Two threads each run a device batch while a third runs single calls; the tensors are zeroed right after their
    call: every output is the single call's."""
    rng = random.Random(77)
    opt = ZopfliOptions(5)
    sets = [[generate(rng.choice("TXMZ"), rng.randrange(1, 100000), 1000 * k + i) for i in range(20)] for k in range(3)]
    want = [[api.compress(f, options=opt, lib=gpu_lib) for f in s] for s in sets]
    tensors = [[_dev(f) for f in s] for s in sets[:2]]
    torch.cuda.synchronize()
    got = [None, None, None]
    errors = []

    def batch(k):
        try:
            got[k] = api.compress_device_batch(tensors[k], options=opt, lib=gpu_lib)
            for t in tensors[k]:
                t.zero_()
        except Exception as e:  # noqa: BLE001 - reported below
            errors.append(repr(e))

    def single():
        try:
            got[2] = [api.compress(f, options=opt, lib=gpu_lib) for f in sets[2]]
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=batch, args=(0,)), threading.Thread(target=batch, args=(1,)),
               threading.Thread(target=single)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    assert not errors, errors
    for k in range(3):
        assert got[k] == want[k], k
