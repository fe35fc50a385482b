"""The device memory pool of a context (zopfli_amd/csrc/device/zmx_pool.h) through its counts (Context.pool_stats,
zmx_internal_pool_stats): what a table build takes comes back, what is cached is accounted to the device once, and trimming
or destroying the context gives it back.  Every test has a context of its own on device 0 beside the session's; the
device's cached total is shared with that one (idle meanwhile), so it is compared by differences.  Integers and digests:
exact."""
import ctypes

import pytest

from zopfli_amd import Context, generate

pytestmark = pytest.mark.gpu

SIZE = 65536
BLOCKS = [(0, SIZE)]


@pytest.fixture(scope="module")
def data():
    return generate("T", SIZE)


def _context(gpu_lib, data):
    ctx = Context(0, gpu_lib)
    at_creation = ctx.pool_stats()
    assert at_creation["cached"] == 0 and at_creation["cached_bytes"] == 0 and at_creation["live"] == 0
    ctx.set_input(data)
    return ctx, at_creation


def test_accounting(gpu_lib, gpu_ctx, data):
    ctx, at_creation = _context(gpu_lib, data)
    try:
        # (the context's own scratch arrays are allocated by its first build and stay: the count is taken after one)
        ctx.build_tables(BLOCKS).free()
        before = ctx.pool_stats()
        t = ctx.build_tables(BLOCKS)
        built = ctx.pool_stats()
        assert built["live"] > before["live"] and built["live_bytes"] > before["live_bytes"]
        t.free()
        freed = ctx.pool_stats()
        assert freed["live"] == before["live"] and freed["live_bytes"] == before["live_bytes"]
        assert freed["cached_bytes"] > 0 and freed["cached"] > 0
        assert freed["device_cached"] - at_creation["device_cached"] == freed["cached_bytes"]
        ctx.trim_cache()
        trimmed = ctx.pool_stats()
        assert trimmed["cached_bytes"] == 0 and trimmed["cached"] == 0
        assert freed["device_cached"] - trimmed["device_cached"] == freed["cached_bytes"]
        assert trimmed["live"] == before["live"]
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def two_builds(gpu_lib, data):
    """Build, free and build the same block again on one context: the counts after each step and the two digests."""
    ctx, at_creation = _context(gpu_lib, data)
    try:
        stats = [ctx.pool_stats()]
        digests = []
        for _ in range(2):
            t = ctx.build_tables(BLOCKS)
            stats.append(ctx.pool_stats())
            digests.append(t.match_digest())
            t.free()
        stats.append(ctx.pool_stats())
        return stats, digests
    finally:
        ctx.close()


def test_reuse(two_builds):
    (start, first, second, _), digests = two_builds
    assert second["from_cache"] - first["from_cache"] >= 1
    assert second["fresh"] - first["fresh"] <= first["fresh"] - start["fresh"]
    assert digests[0] == digests[1]


def test_pinned_buffers(two_builds):
    (_, _, _, end), _ = two_builds
    assert 1 <= end["pinned"] <= 8


def test_destroy_gives_the_cache_back(gpu_lib, gpu_ctx, data):
    ctx, _ = _context(gpu_lib, data)
    try:
        ctx.build_tables(BLOCKS).free()
        held = ctx.pool_stats()
        assert held["cached_bytes"] > 0 and held["live"] > 0      # (live: the input and the match kernel's scratch)
        assert gpu_ctx.pool_stats()["device_cached"] == held["device_cached"]
    finally:
        ctx.close()
    assert held["device_cached"] - gpu_ctx.pool_stats()["device_cached"] == held["cached_bytes"]


def test_set_share_keeps_nothing(gpu_lib, data):
    ctx, _ = _context(gpu_lib, data)
    try:
        ctx.build_tables(BLOCKS).free()
        fn = gpu_lib.zmx_ctx_set_share
        fn.argtypes = [ctypes.c_void_p, ctypes.c_uint]
        fn.restype = ctypes.c_int
        before = ctx.pool_stats()
        assert fn(ctx.handle, 3) == 0
        assert ctx.pool_stats() == before
        assert fn(None, 3) != 0 and b"zmx_ctx_set_share: no context" in gpu_lib.zmx_last_error()
    finally:
        ctx.close()


def test_create_refuses_a_device_that_is_not_there(gpu_lib):
    with pytest.raises(RuntimeError, match="zmx_ctx_create: no such HIP device"):
        Context(-1, gpu_lib)
