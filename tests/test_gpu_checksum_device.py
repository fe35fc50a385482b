"""zmx_checksum_device: CRC-32 and Adler-32 of ranges of arbitrary device memory, pieces and finish on the device
(device/zmx_checksum_device.h), against zlib.  The ranges lie in a uint8 tensor between two guards of 64 bytes of 0xA5, at
every start alignment 0 .. 15 with the lengths around a word and a lane, and at starts 0, 1, 3 with the lengths around a
piece of 256 KiB; contents of zeros, 0xFF (Adler's sums at their largest) and random bytes.  All ranges of one content go
through ONE call, so the call with many ranges — adjacent inside a word, in different tensors, empty — is the usual one."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

from zopfli_amd import Context

pytestmark = pytest.mark.gpu

ZMX_ERR_REFUSED = 3
CRC32, ADLER32 = 0, 1
GUARD = 64
PIECE = 262144
SHORT = [0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 1023, 1024, 1025]
LONG = [PIECE - 1, PIECE, PIECE + 1, 2 * PIECE + 5]
BODY = 2 * PIECE + 5 + 16 + 1025   # room for every (start, length) below


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    c = Context(0, gpu_lib)
    yield c
    c.close()


def _body(fill):
    if fill == "zeros":
        return np.zeros(BODY, dtype=np.uint8)
    if fill == "ones":
        return np.full(BODY, 0xff, dtype=np.uint8)
    return np.random.default_rng(5).integers(0, 256, size=BODY, dtype=np.uint8)


def _guarded(body):
    host = np.concatenate([np.full(GUARD, 0xa5, np.uint8), body, np.full(GUARD, 0xa5, np.uint8)])
    dev = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    return host, dev


def _want(kind, data):
    return (zlib.crc32(data) if kind == CRC32 else zlib.adler32(data)) & 0xffffffff


@pytest.mark.parametrize("fill", ["zeros", "ones", "random"])
@pytest.mark.parametrize("kind", [CRC32, ADLER32], ids=["crc32", "adler32"])
def test_alignments_and_lengths(ctx, kind, fill):
    host, dev = _guarded(_body(fill))
    assert dev.data_ptr() % 16 == 0   # (so a start below is the range's absolute alignment)
    spans = [(GUARD + start, n) for start in range(16) for n in SHORT] + [(GUARD + start, n) for start in (0, 1, 3) for n in LONG]
    got = ctx.checksum_device(kind, [(dev.data_ptr() + at, n) for at, n in spans])
    for (at, n), value in zip(spans, got):
        assert value == _want(kind, host[at:at + n].tobytes()), (kind, fill, at - GUARD, n)
    assert np.array_equal(dev.cpu().numpy(), host), "the buffer changed"


@pytest.mark.parametrize("kind", [CRC32, ADLER32], ids=["crc32", "adler32"])
def test_one_call_with_mixed_ranges(ctx, kind):
    host, dev = _guarded(_body("random"))
    other_host = np.random.default_rng(6).integers(0, 256, size=3001, dtype=np.uint8)
    other = torch.from_numpy(other_host).cuda()
    torch.cuda.synchronize()
    p, q = dev.data_ptr() + GUARD, other.data_ptr()
    # (pointer, bytes, the host's copy)
    ranges = [(p + 1, 1, host[GUARD + 1:GUARD + 2]), (p + 2, 2, host[GUARD + 2:GUARD + 4]),   # adjacent inside one 4-byte word
              (q, 3001, other_host), (q + 5, 0, other_host[:0]), (0, 0, host[:0]), (q + 7, 1500, other_host[7:1507])]
    rng = np.random.default_rng(7)
    for k in range(34):
        n = [0, 1, 3, 17, 1023, 1025, 4097, PIECE + 1][k % 8]
        at = int(rng.integers(0, BODY - n + 1))
        ranges.append((p + at, n, host[GUARD + at:GUARD + at + n]))
    ranges.append((p, 2 * PIECE + 5, host[GUARD:GUARD + 2 * PIECE + 5]))
    assert len(ranges) == 41 and sum(1 for r in ranges if r[1] == 0) >= 5
    got = ctx.checksum_device(kind, [(r[0], r[1]) for r in ranges])
    assert got == [_want(kind, r[2].tobytes()) for r in ranges]
    assert ctx.checksum_device(kind, [dev, other]) == [_want(kind, host.tobytes()), _want(kind, other_host.tobytes())]   # tensors as they are
    assert ctx.checksum_device(kind, []) == []
    assert np.array_equal(dev.cpu().numpy(), host) and np.array_equal(other.cpu().numpy(), other_host), "a buffer changed"


def _managed(nbytes):
    """(pointer, free) of managed memory from the HIP runtime; nothing touches it."""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMallocManaged.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t, ctypes.c_uint]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    p = ctypes.c_void_p()
    assert hip.hipMallocManaged(ctypes.byref(p), nbytes, 1) == 0
    return p.value, lambda: hip.hipFree(p)


def test_refusals_name_their_range(ctx, gpu_lib):
    lib = gpu_lib
    managed, free_managed = _managed(4096)
    dev = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    on_host = np.zeros(4096, dtype=np.uint8)
    torch.cuda.synchronize()
    p = dev.data_ptr()
    fn = lib.zmx_checksum_device
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t),
                   ctypes.POINTER(ctypes.c_uint32)]
    fn.restype = ctypes.c_int
    good = (p, 100)
    refused = [
        ("null pointer with bytes", [good, (None, 4)], 1),
        ("host memory", [good, good, (on_host.ctypes.data, 16)], 2),
        ("leaves its allocation", [(p + 4000, 1 << 40), good], 0),   # (far: the tensor lies in a larger block of its allocator's)
        ("leaves its allocation, behind a good one", [good, (p, 1 << 40)], 1),
        ("managed memory", [good, good, good, (managed, 64)], 3),
    ]
    if torch.cuda.device_count() > 1:
        far = torch.zeros(64, dtype=torch.uint8, device="cuda:1")
        torch.cuda.synchronize(1)
        refused.append(("another device", [good, (far.data_ptr(), 64)], 1))
    for what, ranges, bad in refused:
        n = len(ranges)
        ptrs = (ctypes.c_void_p * n)(*[r[0] for r in ranges])
        sizes = (ctypes.c_size_t * n)(*[r[1] for r in ranges])
        values = (ctypes.c_uint32 * n)(*[0xdeadbeef] * n)
        for kind in (CRC32, ADLER32):
            assert fn(ctx.handle, kind, n, ptrs, sizes, values) != 0, what
            assert lib.zmx_last_error_class() == ZMX_ERR_REFUSED, (what, lib.zmx_last_error())
            assert f"range {bad}".encode() in lib.zmx_last_error(), (what, lib.zmx_last_error())
            assert list(values) == [0xdeadbeef] * n, what
    free_managed()
    # what names no range: an unknown kind, a null array
    ptrs, sizes, values = (ctypes.c_void_p * 1)(p), (ctypes.c_size_t * 1)(100), (ctypes.c_uint32 * 1)(0xdeadbeef)
    for args in ((7, 1, ptrs, sizes, values), (CRC32, 1, None, sizes, values), (CRC32, 1, ptrs, None, values), (CRC32, 1, ptrs, sizes, None)):
        assert fn(ctx.handle, *args) != 0 and lib.zmx_last_error_class() == ZMX_ERR_REFUSED, args[:2]
        assert values[0] == 0xdeadbeef
    assert fn(ctx.handle, CRC32, 0, None, None, None) == 0
    assert fn(ctx.handle, CRC32, 1, ptrs, sizes, values) == 0 and values[0] == zlib.crc32(b"\x00" * 100)
