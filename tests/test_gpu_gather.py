"""zmx_gather_device (k_gather, zopfli_amd/csrc/device/zmx_gather.h): n ranges of device memory put end to end, against
numpy's concatenation over the table of tests/gather_cases.py.  The sources are slices of one allocation at the table's
addresses mod 16; the destination has 64 guard bytes of 0xA5 on both sides, and the sources must be unchanged."""
import numpy as np
import pytest
import torch

import gather_cases as gc
from zopfli_amd import Context

pytestmark = pytest.mark.gpu

ZMX_ERR_REFUSED = 3
CASES = gc.cases()


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    c = Context(0, gpu_lib)
    yield c
    c.close()


def _arena(pieces, device="cuda:0"):
    """The pieces in one allocation, piece i at the next 16-byte boundary plus its address mod 16: the tensor, its host
    image and the (pointer, nbytes) pairs."""
    offsets, at = [], 0
    for s, n in pieces:
        at = (at + 15) // 16 * 16
        offsets.append(at + s)
        at += s + n
    host = np.full(max(at, 1), 0x5A, dtype=np.uint8)
    for i, ((_, n), o) in enumerate(zip(pieces, offsets)):
        host[o:o + n] = gc.piece_bytes(i, n)
    t = torch.from_numpy(host).to(device)
    assert t.data_ptr() % 16 == 0
    return t, host, [(t.data_ptr() + o, n) for (_, n), o in zip(pieces, offsets)]


def _destination(total, dst_mod):
    whole = torch.full((gc.GUARD + 16 + total + gc.GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    assert whole.data_ptr() % 16 == 0
    return whole, gc.GUARD + dst_mod


def _check(whole, at, want):
    got = whole.cpu().numpy()
    assert np.array_equal(got[at:at + len(want)], want)
    assert np.all(got[:at] == 0xA5) and np.all(got[at + len(want):] == 0xA5), "written outside the destination"


@pytest.mark.parametrize("name,dst_mod,pieces", CASES, ids=[c[0] for c in CASES])
def test_gather(ctx, name, dst_mod, pieces):
    arena, host, srcs = _arena(pieces)
    want = gc.expected(pieces)
    whole, at = _destination(len(want), dst_mod)
    torch.cuda.synchronize()
    ctx.gather_device(srcs, whole.data_ptr() + at)
    _check(whole, at, want)
    assert np.array_equal(arena.cpu().numpy(), host), "a source changed"


def test_every_destination_offset(ctx):
    pieces = [((5 * i) % 16, n) for i, n in enumerate(gc.LENGTHS)]
    arena, host, srcs = _arena(pieces)
    want = gc.expected(pieces)
    for dst_mod in range(16):
        whole, at = _destination(len(want), dst_mod)
        torch.cuda.synchronize()
        ctx.gather_device(srcs, whole.data_ptr() + at)
        _check(whole, at, want)
    assert np.array_equal(arena.cpu().numpy(), host)


def test_tensors_of_several_allocations(ctx):
    """Tensors as sources, alternating between allocations (the pointer check asks the runtime again for each)."""
    rng = np.random.default_rng(3)
    hosts = [rng.integers(0, 256, n, dtype=np.uint8) for n in (3000000, 17, 2500000, 70001, 1)]
    tensors = [torch.from_numpy(h).cuda() for h in hosts]
    order = [0, 2, 1, 0, 3, 4, 2]
    want = np.concatenate([hosts[i] for i in order])
    whole, at = _destination(len(want), 9)
    ctx.gather_device([tensors[i] for i in order], whole.data_ptr() + at)
    _check(whole, at, want)
    assert torch.equal(whole[at:at + len(want)], torch.cat([tensors[i] for i in order]))
    with pytest.raises(ValueError):
        ctx.gather_device([tensors[0][::2]], whole.data_ptr() + at)


def test_refusals(ctx, gpu_lib):
    """Refused before any launch (ZMX_ERR_REFUSED), the destination untouched: a host pointer among the sources, a null
    pointer with a size, a destination range that leaves its allocation, a destination that overlaps a source."""
    pieces = [(0, 1000), (3, 50000), (7, 16)]
    arena, host, srcs = _arena(pieces)
    whole, at = _destination(sum(n for _, n in pieces), 0)
    dst = whole.data_ptr() + at
    on_host = np.zeros(4096, dtype=np.uint8)
    big = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda:0")
    small = torch.full((4096,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    refused = [
        ([srcs[0], (on_host.ctypes.data, on_host.size), srcs[2]], dst),
        ([srcs[0], (0, 5)], dst),
        ([(big.data_ptr(), big.numel())] * 512, small.data_ptr()),      # 512 MiB into an allocation of a few MiB at most
        (srcs, arena.data_ptr() + 100),
        (srcs, srcs[1][0] + srcs[1][1] - 1),
    ]
    for bad, d in refused:
        with pytest.raises(RuntimeError):
            ctx.gather_device(bad, d)
        assert gpu_lib.zmx_last_error_class() == ZMX_ERR_REFUSED, gpu_lib.zmx_last_error()
    assert np.all(whole.cpu().numpy() == 0xA5) and np.all(small.cpu().numpy() == 0xA5)
    assert np.array_equal(arena.cpu().numpy(), host)
    ctx.gather_device(srcs, dst)    # and the next valid call is right
    _check(whole, at, gc.expected(pieces))


def test_source_on_another_device(ctx):
    if torch.cuda.device_count() < 2:
        pytest.skip("one visible device")
    pieces = [(1, 5000), (2, 40000), (3, 7)]
    here, _, srcs = _arena(pieces)
    there, there_host, other = _arena(pieces, device="cuda:1")
    mixed = [srcs[0], other[1], srcs[2]]
    want = gc.expected(pieces)
    whole, at = _destination(len(want), 5)
    torch.cuda.synchronize(0)
    torch.cuda.synchronize(1)
    ctx.gather_device(mixed, whole.data_ptr() + at)
    _check(whole, at, want)
    assert np.array_equal(there.cpu().numpy(), there_host)
