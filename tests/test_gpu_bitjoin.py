"""zmx_bitjoin_device (k_bitjoin, zopfli_amd/csrc/device/zmx_bitjoin.h): n bit strings of device memory joined into one,
against the big-integer reference over the tables of tests/bitjoin_cases.py.  The sources are stretches of one allocation
of random bytes at the table's addresses mod 16; the destination is filled with 0xA5 and has 64 guard bytes of 0xA5 on
both sides, so a byte left out shows as well as one written outside; the sources must be unchanged."""
import ctypes

import numpy as np
import pytest
import torch

import bitjoin_cases as bc
from zopfli_amd import Context

pytestmark = pytest.mark.gpu

ZMX_ERR_REFUSED = 3
GUARD = 64
CASES = bc.cases()


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    c = Context(0, gpu_lib)
    yield c
    c.close()


def _destination(nbytes, dst_mod, device="cuda:0"):
    whole = torch.full((GUARD + 16 + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=device)
    assert whole.data_ptr() % 16 == 0
    return whole, GUARD + dst_mod


def _check(whole, at, want):
    got = whole.cpu().numpy()
    assert np.array_equal(got[at:at + len(want)], want)
    assert np.all(got[:at] == 0xA5) and np.all(got[at + len(want):] == 0xA5), "written outside the destination"


def _join(ctx, case):
    name, dst_mod, total_bits, pieces = case
    host = bc.arena(name, pieces)
    arena = torch.from_numpy(host).cuda()
    assert arena.data_ptr() % 16 == 0
    want = bc.expected(total_bits, pieces, host)
    whole, at = _destination(len(want), dst_mod)
    torch.cuda.synchronize()
    table = [(0 if off is None else arena.data_ptr() + off, sb, nb, db) for off, sb, nb, db in pieces]
    ctx.bitjoin_device(table, total_bits, whole.data_ptr() + at, len(want))
    _check(whole, at, want)
    assert np.array_equal(arena.cpu().numpy(), host), "a source changed"


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_bitjoin(ctx, case):
    _join(ctx, case)


def test_past_the_grid(ctx):
    """33 MiB + 5 bits from two pieces with odd shifts: more tiles than the grid's 2048 workgroups."""
    case = bc.big()
    assert (case[2] + 7) // 8 > 2048 * bc.TILE
    _join(ctx, case)


def _managed(nbytes):
    """(pointer, free) of managed memory from the HIP runtime; nothing touches it."""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMallocManaged.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t, ctypes.c_uint]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    p = ctypes.c_void_p()
    assert hip.hipMallocManaged(ctypes.byref(p), nbytes, 1) == 0
    return p.value, lambda: hip.hipFree(p)


def test_refusals(ctx, gpu_lib):
    """Refused before any launch (ZMX_ERR_REFUSED), the message naming the piece where one is at fault, the destination
    untouched; after each refusal the next valid call is right."""
    host = np.random.default_rng(5).integers(0, 256, 1 << 16, dtype=np.uint8)
    arena = torch.from_numpy(host).cuda()
    a = arena.data_ptr()
    good = [(a + 3, 5, 1000, 0), (a + 4096, 1, 70000, 1003)]
    total = 71003
    nbytes = (total + 7) // 8
    want = bc.expected(total, [(3, 5, 1000, 0), (4096, 1, 70000, 1003)], host)
    whole, at = _destination(nbytes, 5)
    dst = whole.data_ptr() + at
    on_host = np.zeros(1 << 16, dtype=np.uint8)
    managed, free_managed = _managed(1 << 16)
    torch.cuda.synchronize()
    refused = [
        ("piece 1: null pointer", [good[0], (0, 0, 5, 1003)], total, dst, nbytes),
        ("piece 1", [good[0], (on_host.ctypes.data, 1, 70000, 1003)], total, dst, nbytes),              # host memory
        ("piece 0", [(managed, 5, 1000, 0), good[1]], total, dst, nbytes),                                 # managed memory
        ("the destination", good, total, on_host.ctypes.data, nbytes),
        ("the destination", good, total, managed, nbytes),
        ("piece 1", [good[0], (a, 1 << 40, 70000, 1003)], total, dst, nbytes),                             # leaves its allocation
        ("the destination", good[:1], 1 << 45, dst, 1 << 42),
        ("piece 1: the destination overlaps this source", [good[0], (dst + nbytes - 1, 7, 1, 1003)], total, dst, nbytes),
        ("piece 0: the destination overlaps this source", good, total, a + 100, nbytes),
        ("piece 1: the pieces are not sorted", [good[1], good[0]], total + 1003, dst, nbytes + 200),
        ("piece 1: it overlaps the piece before it", [good[0], (a + 4096, 1, 70000, 999)], total, dst, nbytes),
        ("below the last piece's end", good, total - 1, dst, nbytes),
        ("above 8 * dst_capacity", good, 8 * nbytes + 1, dst, nbytes),
        ("above 8 * dst_capacity", good, total, dst, nbytes - 1),
    ]
    try:
        for text, pieces, bits, d, cap in refused:
            with pytest.raises(RuntimeError) as e:
                ctx.bitjoin_device(pieces, bits, d, cap)
            assert text in str(e.value), (text, str(e.value))
            assert gpu_lib.zmx_last_error_class() == ZMX_ERR_REFUSED, gpu_lib.zmx_last_error()
            assert np.all(whole.cpu().numpy() == 0xA5), text
            ctx.bitjoin_device(good, total, dst, nbytes)      # and the next valid call is right
            _check(whole, at, want)
            whole.fill_(0xA5)
            torch.cuda.synchronize()
        assert np.array_equal(arena.cpu().numpy(), host)
    finally:
        free_managed()


def test_total_bits_zero_launches_nothing(ctx):
    whole, at = _destination(16, 3)
    torch.cuda.synchronize()
    ctx.bitjoin_device([], 0, whole.data_ptr() + at, 0)
    ctx.bitjoin_device([(0, 0, 0, 0)], 0, 0, 0)       # (no destination at all: nothing is asked of it)
    assert np.all(whole.cpu().numpy() == 0xA5)


def test_another_device(ctx):
    """A source on another device, a destination that is not on the context's."""
    if torch.cuda.device_count() < 2:
        pytest.skip("one visible device")
    here = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    there = torch.zeros(4096, dtype=torch.uint8, device="cuda:1")
    torch.cuda.synchronize(0)
    torch.cuda.synchronize(1)
    with pytest.raises(RuntimeError, match="piece 0: the source is not memory of the context's device"):
        ctx.bitjoin_device([(there.data_ptr(), 0, 100, 0)], 100, here.data_ptr(), 4096)
    with pytest.raises(RuntimeError, match="the destination is not memory of the context's device"):
        ctx.bitjoin_device([(here.data_ptr(), 0, 100, 0)], 100, there.data_ptr(), 4096)
