"""zmx_bitjoin_many_device (k_bitjoin_many, zopfli_amd/csrc/device/zmx_bitjoin.h): many destinations joined in one launch,
over the tables of tests/bitjoin_many_cases.py against the big-integer reference applied per destination.  The
destinations are slices of one torch allocation filled with 0xA5, 64 guard bytes on both sides; every byte outside the
destinations must still be 0xA5 afterwards, and the sources unchanged."""
import ctypes

import numpy as np
import pytest
import torch

import bitjoin_cases as bc
import bitjoin_many_cases as mc
from zopfli_amd import Context

pytestmark = pytest.mark.gpu

ZMX_ERR_REFUSED = 3
GUARD = 64
CASES = mc.cases()


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    c = Context(0, gpu_lib)
    yield c
    c.close()


def _tables(case, block_ptr, arena_ptr):
    """(dests, pieces) of a case whose block begins at block_ptr (16-byte aligned) and whose sources at arena_ptr."""
    dests, pieces = [], []
    for at, (_, total_bits, ps) in zip(mc.positions(case)[0], case[3]):
        dests.append((block_ptr + at, total_bits, len(pieces), len(ps)))
        pieces += [(0 if off is None else arena_ptr + off, sb, nb, db) for off, sb, nb, db in ps]
    return dests, pieces


def _join(ctx, case):
    host = case[4]
    arena = torch.from_numpy(host).cuda()
    want = mc.expected_block(case)
    whole = torch.full((GUARD + len(want) + GUARD,), mc.CANARY, dtype=torch.uint8, device="cuda:0")
    assert arena.data_ptr() % 16 == 0 and whole.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    dests, pieces = _tables(case, whole.data_ptr() + GUARD, arena.data_ptr())
    ctx.bitjoin_many_device(dests, pieces)
    got = whole.cpu().numpy()
    bad = np.flatnonzero(got[GUARD:GUARD + len(want)] != want)
    assert bad.size == 0, (case[0], bad[:8])
    assert np.all(got[:GUARD] == mc.CANARY) and np.all(got[GUARD + len(want):] == mc.CANARY), "written outside the block"
    assert np.array_equal(arena.cpu().numpy(), host), "a source changed"


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_bitjoin_many(ctx, case):
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
    """Refused before any upload or launch (ZMX_ERR_REFUSED), the message naming the destination and the piece at fault,
    the block untouched; after each refusal the next valid call is right."""
    host = np.random.default_rng(6).integers(0, 256, 1 << 16, dtype=np.uint8)
    arena = torch.from_numpy(host).cuda()
    a = arena.data_ptr()
    # destinations of 5, 1 and 27 bytes back to back, 3 bytes past a 16-byte boundary
    local = [[(3, 5, 33, 0), (100, 1, 7, 33)], [(200, 2, 8, 0)], [(4096, 7, 100, 0), (8192, 0, 116, 100)]]
    totals = [40, 8, 216]
    whole = torch.full((GUARD + 16 + 33 + GUARD,), mc.CANARY, dtype=torch.uint8, device="cuda:0")
    base = whole.data_ptr() + GUARD + 3
    at = [0, 5, 6]
    want = np.full(len(whole), mc.CANARY, dtype=np.uint8)
    for o, tb, ps in zip(at, totals, local):
        want[GUARD + 3 + o:GUARD + 3 + o + tb // 8] = bc.expected(tb, ps, host)
    pieces = [(a + off, sb, nb, db) for ps in local for off, sb, nb, db in ps]
    dests = [(base, 40, 0, 2), (base + 5, 8, 2, 1), (base + 6, 216, 3, 2)]
    on_host = np.zeros(1 << 12, dtype=np.uint8)
    managed, free_managed = _managed(1 << 12)
    torch.cuda.synchronize()

    def with_piece(i, piece):
        return pieces[:i] + [piece] + pieces[i + 1:]

    def with_dest(i, dest):
        return dests[:i] + [dest] + dests[i + 1:]

    refused = [
        ("destination 1: its pieces do not follow", with_dest(1, (base + 5, 8, 1, 1)), pieces, None),
        ("destination 2: its pieces leave the table", with_dest(2, (base + 6, 216, 3, 3)), pieces, None),
        ("the destinations take 3 pieces of 5", dests[:2], pieces, None),
        ("destination 0: piece 1: it overlaps the piece before it", dests, with_piece(1, (a + 100, 1, 7, 32)), None),
        ("destination 2: piece 0: null pointer", dests, with_piece(3, (0, 7, 100, 0)), None),
        ("destination 2: total_bits 215 is below the last piece's end", with_dest(2, (base + 6, 215, 3, 2)), pieces, None),
        ("destination 0: total_bits 40 is above 8 * dst_capacity", dests, pieces, [4, 1, 27]),
        ("destination 1 overlaps destination 0", with_dest(1, (base + 4, 8, 2, 1)), pieces, None),
        ("destination 2 overlaps destination 1", with_dest(2, (base + 5, 216, 3, 2)), pieces, None),
        ("destination 0: piece 0: destination 2 overlaps this source", dests, with_piece(0, (base + 32, 0, 33, 0)), None),
        ("destination 1: piece 0: destination 1 overlaps this source", dests, with_piece(2, (base + 4, 8, 8, 0)), None),
        ("destination 1", with_dest(1, (on_host.ctypes.data, 8, 2, 1)), pieces, None),                        # host memory
        ("destination 2", with_dest(2, (managed, 216, 3, 2)), pieces, None),                                  # managed memory
        ("destination 2", with_dest(2, (base + 6, 1 << 50, 3, 2)), pieces, None),                             # leaves its allocation
        ("destination 2: piece 1", dests, with_piece(4, (on_host.ctypes.data, 0, 116, 100)), None),
        ("destination 0: piece 0", dests, with_piece(0, (managed, 5, 33, 0)), None),
        ("destination 2: piece 1", dests, with_piece(4, (a, 1 << 40, 116, 100)), None),                       # leaves its allocation
    ]
    try:
        for text, d, p, caps in refused:
            with pytest.raises(RuntimeError) as e:
                ctx.bitjoin_many_device(d, p, caps)
            assert text in str(e.value), (text, str(e.value))
            assert gpu_lib.zmx_last_error_class() == ZMX_ERR_REFUSED, gpu_lib.zmx_last_error()
            assert np.all(whole.cpu().numpy() == mc.CANARY), text
            ctx.bitjoin_many_device(dests, pieces, [5, 1, 27])      # and the next valid call is right
            assert np.array_equal(whole.cpu().numpy(), want), text
            whole.fill_(mc.CANARY)
            torch.cuda.synchronize()
        with pytest.raises(RuntimeError, match="null destination table"):
            _raw_null(ctx)
        assert gpu_lib.zmx_last_error_class() == ZMX_ERR_REFUSED
        assert np.array_equal(arena.cpu().numpy(), host)
    finally:
        free_managed()


def _raw_null(ctx):
    """A null destination table with a count of 2, which Context.bitjoin_many_device cannot express."""
    fn = ctx.lib.zmx_bitjoin_many_device
    fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t), ctypes.c_size_t, ctypes.c_void_p]
    fn.restype = ctypes.c_int
    if fn(ctx.handle, 2, None, None, 0, None) != 0:
        raise RuntimeError((ctx.lib.zmx_last_error() or b"").decode())


def test_no_destination_launches_nothing(ctx, gpu_lib):
    whole = torch.full((256,), mc.CANARY, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    gpu_lib.zmx_set_kernel_timing(1)
    try:
        fn = gpu_lib.zmx_internal_bitjoin_ms
        fn.restype = ctypes.c_double
        ctx.bitjoin_many_device([(whole.data_ptr() + 70, 8, 0, 0)], [])     # (a launch: the timer then reads above 0)
        assert fn() > 0
        ctx.bitjoin_many_device([], [])
        assert fn() == 0
        ctx.bitjoin_many_device([(0, 0, 0, 1), (whole.data_ptr() + 3, 0, 1, 0), (0, 0, 1, 0)], [(0, 0, 0, 0)])     # no bit anywhere
        assert fn() == 0
    finally:
        gpu_lib.zmx_set_kernel_timing(0)
    got = whole.cpu().numpy()
    assert got[70] == 0 and np.all(np.delete(got, 70) == mc.CANARY)


def test_another_device(ctx):
    """A source on another device, a destination that is not on the context's."""
    if torch.cuda.device_count() < 2:
        pytest.skip("one visible device")
    here = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    there = torch.zeros(4096, dtype=torch.uint8, device="cuda:1")
    torch.cuda.synchronize(0)
    torch.cuda.synchronize(1)
    with pytest.raises(RuntimeError, match="destination 0: piece 0: the source is not memory of the context's device"):
        ctx.bitjoin_many_device([(here.data_ptr(), 100, 0, 1)], [(there.data_ptr(), 0, 100, 0)])
    with pytest.raises(RuntimeError, match="destination 0 is not memory of the context's device"):
        ctx.bitjoin_many_device([(there.data_ptr(), 100, 0, 1)], [(here.data_ptr(), 0, 100, 0)])
