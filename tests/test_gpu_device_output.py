"""Output that stays in device memory: zmx_compress_device_to_device (api.compress_device_out) against api.compress of the
same bytes and, where tests/golden has the vector, the reference's SHA-256; zmx_last_output_traffic, the capacity rule,
the refusals; and the device layer's two halves — zmx_encode_blocks_device joined by zmx_bitjoin_device — against
zmx_encode_blocks on the stores of test_gpu_bit_writer_limits.py.  Device buffers come from torch; every destination is
filled with 0xA5 and has 64 guard bytes on both sides."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

import steer_cases as sc
from test_gpu_bit_writer_limits import _steered_tables
from zopfli_amd import ZopfliOptions, api, generate

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "vectors.json")
ZMX_ERR_REFUSED = 3
GUARD = 64
FORMATS = [api.FORMAT_GZIP, api.FORMAT_ZLIB, api.FORMAT_DEFLATE]

_inputs = {}
_wants = {}


def _random(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _input(name):
    if name not in _inputs:
        _inputs[name] = {
            "empty": lambda: b"",
            "one": lambda: b"a",
            "T70000": lambda: generate("T", 70000),
            "random65535": lambda: _random(65535, 1),       # a stored block of one piece
            "random65536": lambda: _random(65536, 2),       # ... of two
            "random131071": lambda: _random(131071, 3),
            # stored blocks that start at a bit pointer other than 0
            "thirds300000": lambda: generate("T", 100000) + _random(100000, 4) + generate("T", 100000),
            "T1000001": lambda: generate("T", 1000001),     # the second master block holds one byte
        }[name]()
    return _inputs[name]


INPUTS = ["empty", "one", "T70000", "random65535", "random65536", "random131071", "thirds300000", "T1000001"]


def _want(gpu_lib, name, fmt, splitting):
    key = (name, fmt, splitting)
    if key not in _wants:
        _wants[key] = api.compress(_input(name), fmt, ZopfliOptions(5, splitting), lib=gpu_lib)
    return _wants[key]


def _dev(data):
    if len(data) == 0:
        return torch.empty(0, dtype=torch.uint8, device="cuda")
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def _destination(capacity, offset=0):
    """A destination of `capacity` bytes `offset` bytes behind a 16-byte boundary, everything 0xA5: (allocation, view)."""
    whole = torch.full((GUARD + offset + capacity + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    return whole, whole[GUARD + offset:GUARD + offset + capacity]


def _check(whole, offset, want, capacity):
    got = whole.cpu().numpy()
    at = GUARD + offset
    assert got[at:at + len(want)].tobytes() == want
    assert np.all(got[:at] == 0xA5) and np.all(got[at + len(want):] == 0xA5), "written outside the stream"
    assert len(got) == at + capacity + GUARD


@pytest.mark.parametrize("splitting", [0, 1])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", INPUTS)
def test_equals_host_call(gpu_lib, name, fmt, splitting):
    data = _input(name)
    want = _want(gpu_lib, name, fmt, splitting)
    capacity = len(want) + 100
    whole, dst = _destination(capacity)
    size = api.compress_device_out(_dev(data), dst, fmt, ZopfliOptions(5, splitting), lib=gpu_lib)
    assert size == len(want)
    _check(whole, 0, want, capacity)
    traffic = api.last_output_traffic(gpu_lib)
    assert traffic[0] == 0, traffic
    assert traffic[2] + traffic[3] >= 1 or name.startswith("random") or name == "empty", traffic
    assert len(want) <= api.compress_bound(len(data), fmt, lib=gpu_lib)


def _golden():
    with open(GOLDEN) as f:
        return [c for c in json.load(f) if c["insize"] <= 7013 or (c["insize"] <= 65536 and c["numiterations"] <= 5)]


def _gid(c):
    return (f"{c['input'].get('name', c['input'].get('cls'))}-{c['insize']}-f{c['format']}-n{c['numiterations']}"
            f"-s{c['blocksplitting']}")


@pytest.mark.parametrize("case", _golden(), ids=_gid)
def test_golden(gpu_lib, case):
    """The reference's bytes (SHA-256 of its output, tests/golden/vectors.json), left in device memory."""
    spec = case["input"]
    if spec["kind"] == "literal":
        from golden.make_golden import LITERALS
        data = LITERALS[spec["name"]]
    else:
        data = generate(spec["cls"], spec["size"], spec.get("seed"))
    opt = ZopfliOptions(case["numiterations"], case["blocksplitting"], case["blocksplittingmax"])
    capacity = api.compress_bound(len(data), case["format"], lib=gpu_lib)
    whole, dst = _destination(capacity)
    size = api.compress_device_out(_dev(data), dst, case["format"], opt, lib=gpu_lib)
    assert size == case["outsize"]
    assert hashlib.sha256(dst[:size].cpu().numpy().tobytes()).hexdigest() == case["sha256"]


def test_host_call_reports_its_stream(gpu_lib):
    """For the existing entries [0] is the stream and the rest are 0."""
    out = api.compress(_input("T70000"), api.FORMAT_GZIP, ZopfliOptions(5, 0), lib=gpu_lib)
    assert api.last_output_traffic(gpu_lib) == [float(len(out)), 0.0, 0.0, 0.0]
    out = api.compress_device(_dev(_input("T70000")), fmt=api.FORMAT_ZLIB, options=ZopfliOptions(5, 1), lib=gpu_lib)
    assert api.last_output_traffic(gpu_lib) == [float(len(out)), 0.0, 0.0, 0.0]


def test_traffic_of_one_text_block(gpu_lib):
    """One class-T master block without block splitting: its symbols' bits never leave the device, and what goes up is the
    container's 18 bytes and the block's header and tree — at most 17 + 57 + 320 x 14 bits, below 600 bytes."""
    data = _input("T70000")
    want = _want(gpu_lib, "T70000", api.FORMAT_GZIP, 0)
    whole, dst = _destination(len(want))
    assert api.compress_device_out(_dev(data), dst, api.FORMAT_GZIP, ZopfliOptions(5, 0), lib=gpu_lib) == len(want)
    _check(whole, 0, want, len(want))
    traffic = api.last_output_traffic(gpu_lib)
    print("output traffic:", traffic)
    assert traffic[0] == 0 and traffic[2] == 1 and traffic[3] == 0
    assert 18 < traffic[1] <= 600 + 18


_CHILD = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from zopfli_amd import ZopfliOptions, api, generate
data = generate("T", int(sys.argv[2]))
opt = ZopfliOptions(5, 1)
want = api.compress(data, api.FORMAT_GZIP, opt)
src = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
dst = torch.full((len(want) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
try:
    size = api.compress_device_out(src, dst, api.FORMAT_GZIP, opt)
except RuntimeError as e:
    print("REFUSED", api.library().zmx_last_error_class(), str(e))
    print("UNTOUCHED", bool(torch.all(dst == 0xA5).item()))
    size = api.compress_device_out(src[:70000], dst, api.FORMAT_GZIP, opt)
    print("NEXT", dst[:size].cpu().numpy().tobytes() == api.compress(data[:70000], api.FORMAT_GZIP, opt))
else:
    got = dst.cpu().numpy()
    print("SAME", size == len(want) and got[:size].tobytes() == want and bool(np.all(got[size:] == 0xA5)))
    print("TRAFFIC", *api.last_output_traffic())
"""


def _child(env, nbytes):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(nbytes)], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout, r.stderr[-3000:])
    return {line.split()[0]: line.split()[1:] for line in r.stdout.splitlines() if line.strip()}


def test_host_written_blocks_are_uploaded():
    """ZOPFLI_AMD_DEVICE_ENCODE=0 (its own process: the switch is read once): every block's bits are made on the host and go
    up with the literals — the same bytes."""
    out = _child({"ZOPFLI_AMD_DEVICE_ENCODE": "0"}, 300000)
    assert out["SAME"] == ["True"], out
    traffic = [float(v) for v in out["TRAFFIC"]]
    assert traffic[0] == 0 and traffic[2] == 0 and traffic[3] > 0 and traffic[1] > 1000, traffic


def test_more_than_one_round_is_refused():
    """ZOPFLI_AMD_ROUND_PARTS=1 and 1 000 001 bytes: two rounds, which are not joined on the device."""
    out = _child({"ZOPFLI_AMD_ROUND_PARTS": "1"}, 1000001)
    assert out["REFUSED"][0] == str(ZMX_ERR_REFUSED) and "round" in " ".join(out["REFUSED"]), out
    assert out["UNTOUCHED"] == ["True"] and out["NEXT"] == ["True"], out


@pytest.mark.parametrize("name,splitting", [("T70000", 1), ("random131071", 0), ("thirds300000", 1)])
def test_capacity(gpu_lib, name, splitting):
    """Capacity equal to the size passes; one less is refused with the size reported and nothing written; zmx_compress_bound passes."""
    data = _input(name)
    want = _want(gpu_lib, name, api.FORMAT_GZIP, splitting)
    opt = ZopfliOptions(5, splitting)
    src = _dev(data)
    whole, dst = _destination(len(want))
    assert api.compress_device_out(src, dst, api.FORMAT_GZIP, opt, lib=gpu_lib) == len(want)
    _check(whole, 0, want, len(want))
    whole, dst = _destination(len(want) - 1)
    with pytest.raises(api.CapacityError) as e:
        api.compress_device_out(src, dst, api.FORMAT_GZIP, opt, lib=gpu_lib)
    assert e.value.needed == len(want)
    assert gpu_lib.zmx_last_error_class() == ZMX_ERR_REFUSED
    assert np.all(whole.cpu().numpy() == 0xA5)
    bound = api.compress_bound(len(data), api.FORMAT_GZIP, lib=gpu_lib)
    whole, dst = _destination(bound)
    assert api.compress_device_out(src, dst, api.FORMAT_GZIP, opt, lib=gpu_lib) == len(want)
    _check(whole, 0, want, bound)


def test_refusals(gpu_lib):
    """d_out in host memory, managed, null, overlapping d_in, leaving its allocation: refused (ZMX_ERR_REFUSED), nothing
    written, and the next valid call is right."""
    data = _input("T70000")
    opt = ZopfliOptions(5, 0)
    want = _want(gpu_lib, "T70000", api.FORMAT_GZIP, 0)
    capacity = len(want) + 10
    room = torch.full((len(data) + capacity,), 0xA5, dtype=torch.uint8, device="cuda")
    src = room[:len(data)]
    src.copy_(_dev(data))
    on_host = np.full(capacity, 0xA5, dtype=np.uint8)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMallocManaged.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t, ctypes.c_uint]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    managed = ctypes.c_void_p()
    assert hip.hipMallocManaged(ctypes.byref(managed), capacity, 1) == 0
    whole, dst = _destination(capacity)
    torch.cuda.synchronize()
    try:
        refused = [
            (on_host.ctypes.data, capacity),
            (managed.value, capacity),
            (0, capacity),
            (src.data_ptr() + len(data) - 1, capacity),      # its first byte is d_in's last
            (src.data_ptr() + 100, 50),                      # inside d_in
            (dst.data_ptr(), 1 << 40),                       # leaves its allocation
        ]
        for d in refused:
            with pytest.raises(RuntimeError) as e:
                api.compress_device_out(src, d, api.FORMAT_GZIP, opt, lib=gpu_lib)
            assert not isinstance(e.value, api.CapacityError), d
            assert gpu_lib.zmx_last_error_class() == ZMX_ERR_REFUSED, gpu_lib.zmx_last_error()
            assert np.all(on_host == 0xA5) and np.all(whole.cpu().numpy() == 0xA5)
            assert room[:len(data)].cpu().numpy().tobytes() == data and bool(torch.all(room[len(data):] == 0xA5).item())
            assert api.compress_device_out(src, dst, api.FORMAT_GZIP, opt, lib=gpu_lib) == len(want)
            _check(whole, 0, want, capacity)
            whole.fill_(0xA5)
            torch.cuda.synchronize()
        with pytest.raises(ValueError):
            api.compress_device_out(src, whole[::2], api.FORMAT_GZIP, opt, lib=gpu_lib)
    finally:
        hip.hipFree(managed)


@pytest.mark.parametrize("name,splitting", [("T70000", 1), ("random65536", 0)])
def test_destination_view_at_offset_3(gpu_lib, name, splitting):
    want = _want(gpu_lib, name, api.FORMAT_GZIP, splitting)
    whole, dst = _destination(len(want) + 5, offset=3)
    assert dst.data_ptr() % 16 == 3
    assert api.compress_device_out(_dev(_input(name)), dst, api.FORMAT_GZIP, ZopfliOptions(5, splitting), lib=gpu_lib) == len(want)
    _check(whole, 3, want, len(want) + 5)


def test_concurrent_callers(gpu_lib):
    """Four threads at once, each with buffers of its own, two rounds each."""
    names = [("T70000", 1), ("random131071", 0), ("thirds300000", 1), ("T1000001", 0)]
    wants = [_want(gpu_lib, n, api.FORMAT_GZIP, s) for n, s in names]
    srcs = [_dev(_input(n)) for n, _ in names]
    dsts = [_destination(len(w) + 7) for w in wants]
    torch.cuda.synchronize()
    errors = []

    def work(i):
        try:
            for _ in range(2):
                size = api.compress_device_out(srcs[i], dsts[i][1], api.FORMAT_GZIP, ZopfliOptions(5, names[i][1]), lib=gpu_lib)
                assert size == len(wants[i])
                _check(dsts[i][0], 0, wants[i], len(wants[i]) + 7)
        except BaseException as e:   # noqa: BLE001 (reported below, on the test's thread)
            errors.append((i, repr(e)))
    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(names))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def _device_layer_jobs(name):
    """The jobs of test_gpu_bit_writer_limits.py's cases on the steered store `name`: [(block, litlens, dists, codes, bit_start)]."""
    c = sc.steered(name)
    jobs = []
    if name == "literals":
        for b, (la, ll, dd) in enumerate(c["runs"]):
            jobs.append((b, ll, dd, sc.codes_15bit(30 + b), (0, 3, 77, 31, 64)[b]))
            jobs.append((b, ll, dd, sc.codes_mixed(40 + b), (17, 0, 1, 4099, 5)[b]))
            jobs.append((b, ll, dd, sc.codes_sparse(ll, dd, 50 + b), (8, 9, 0, 2, 30)[b]))
    else:
        la, ll, dd = c["runs"][0]
        jobs += [(0, ll, dd, sc.codes_15bit(11), start) for start in (0, 1, 7, 31, 4100)]
        jobs += [(0, ll, dd, sc.codes_mixed(12), 7), (0, ll, dd, sc.codes_sparse(ll, dd, 13), 0), (0, ll[:1000], dd[:1000], sc.codes_15bit(14), 63)]
    return jobs


@pytest.mark.parametrize("name", ["tile48", "tile48_mixed", "literals"])
def test_device_layer_reproduces_encode_blocks(gpu_ctx, name):
    """zmx_encode_blocks_device + zmx_bitjoin_device against zmx_encode_blocks, bit for bit: every job's whole string —
    the zero bits in front of bit_start included — joined at a ragged bit offset into one destination."""
    t, c, nsym = _steered_tables(gpu_ctx, name)
    bits = None
    try:
        jobs = _device_layer_jobs(name)
        call = []
        for block, ll, dd, codes, start in jobs:
            nbits = int(sc.symbol_bits(ll, dd, codes).sum()) + (int(codes[256]) >> 16)
            call.append((block, 1, len(ll), start, nbits))
        codes = np.stack([j[3] for j in jobs])
        host = t.encode_blocks(call, codes)
        bits = t.encode_blocks_device(call, codes)
        pieces, acc, cur = [], 0, 5
        for j, (h, (_, _, _, start, nbits)) in enumerate(zip(host, call)):
            ptr, got_start, got_nbits = bits.job(j)
            assert (got_start, got_nbits) == (start, nbits) and ptr % 8 == 0
            whole_bits = start + nbits
            assert int.from_bytes(h, "little") >> whole_bits == 0 and int.from_bytes(h, "little") & ((1 << start) - 1) == 0
            pieces.append((ptr, 0, whole_bits, cur))
            acc |= int.from_bytes(h, "little") << cur
            cur += whole_bits + (j % 5)
        want = np.frombuffer(acc.to_bytes((cur + 7) // 8, "little"), dtype=np.uint8)
        whole, dst = _destination(len(want), offset=1)
        torch.cuda.synchronize()
        gpu_ctx.bitjoin_device(pieces, cur, dst.data_ptr(), len(want))
        _check(whole, 1, want.tobytes(), len(want))
    finally:
        if bits is not None:
            bits.free()
        t.free()
