"""What k_verify REPORTS (zmx_verify_stores, zmx_encode.h): the header and Tables.verify_stores promise the first
offending block and symbol, and the reason.  The reference is steer_cases.verify_len_dist, ZopfliVerifyLenDist
(lz77.c:270-295) over a downloaded store in plain Python, which returns the first failing symbol and why.

Tables are built on input A and hold a greedy and an optimal store per block; then zmx_set_input puts B in A's place —
the same length, so the resident buffer is reused — which differs from A in bytes chosen from the store's cumulative
positions, so that the first failing symbol is the one aimed at: a literal, a match whose own bytes changed, a match
of which only the source (in the window before the block) changed; at index 0, 63, 64 (the wave's edge), 255, 256, 257
(the 256-symbol chunk's edge) and the last symbol of a partial chunk.  Every B carries LATER failures too — the next
symbol, one in the next chunk, the last one — so a kernel that kept the last failing symbol instead of the first fails.

Reason 1 (length or distance out of range) cannot be provoked through the C ABI: no entry point uploads a store, and
the stores the kernels write are in range.  It is left out.  Input A is restored after every case (gpu_ctx is
session-scoped).  Integer and string equality, no tolerance."""
import re

import numpy as np
import pytest

import oracle_lib as ol
import steer_cases as sc
from zopfli_amd import generate

pytestmark = pytest.mark.gpu

BLOCKS = [(0, 70000), (70000, 200000)]
MSG = re.compile(r"zmx_verify_stores: block (\d+), symbol (\d+): (.*)$")
REASON = {2: "the bytes it stands for are not the input's", 3: "the symbols do not add up to the block"}
STORES = [(0, 0), (0, 1), (1, 0), (1, 1)]                # (block, slot): slot 0 greedy, slot 1 optimal
TARGETS = [0, 63, 64, 255, 256, 257, "last"]


@pytest.fixture(scope="module")
def verify_case(gpu_ctx):
    """(A, Tables, {(block, slot): (litlens, dists)}): greedy stores in slot 0, one optimal run in slot 1; all pass on A."""
    a = generate("M", BLOCKS[-1][1])
    gpu_ctx.set_input(a)
    t = gpu_ctx.build_tables(BLOCKS)
    nsym, hist = t.greedy(0)
    cost, mincost = sc.cost_rows([ol.entropy_costs(h) for h in hist])
    nsym2, _ = t.squeeze_run(cost, mincost, np.ones(len(BLOCKS), dtype=np.int32))
    stores = {}
    for b in range(len(BLOCKS)):
        stores[(b, 0)] = t.store(b, 0, nsym[b])
        stores[(b, 1)] = t.store(b, 1, nsym2[b])
    t.verify_stores([0, 1], [0, 0], nsym)
    t.verify_stores([0, 1], [1, 1], nsym2)
    for (b, slot), (ll, dd) in stores.items():
        assert sc.verify_len_dist(a, *BLOCKS[b], ll, dd) is None
        assert len(ll) % 256 not in (0, 1) and len(ll) > 600           # the last chunk is a partial one
    yield a, t, stores
    gpu_ctx.set_input(a)
    t.free()


def _positions(block, ll, dd):
    """First byte of every symbol of a store."""
    lens = np.where(dd == 0, 1, ll).astype(np.int64)
    return BLOCKS[block][0] + np.cumsum(lens) - lens, lens


def _flip(a, places):
    b = bytearray(a)
    for p in places:
        b[p] ^= 0xff
    return bytes(b)


def _report(gpu_ctx, t, a, b, jobs):
    """The failure zmx_verify_stores reports for `jobs` = [(block, slot, nsym)] against input b: (block, symbol, text),
    or None when it passes.  A is back in place afterwards."""
    gpu_ctx.set_input(b)
    try:
        t.verify_stores([j[0] for j in jobs], [j[1] for j in jobs], [j[2] for j in jobs])
        return None
    except RuntimeError as e:
        m = MSG.search(str(e))
        assert m, str(e)
        return int(m.group(1)), int(m.group(2)), m.group(3)
    finally:
        gpu_ctx.set_input(a)


@pytest.mark.parametrize("target", TARGETS, ids=str)
@pytest.mark.parametrize("store", STORES, ids=lambda s: f"block{s[0]}-{'greedy' if s[1] == 0 else 'optimal'}")
def test_first_failing_symbol(gpu_ctx, verify_case, store, target):
    """A byte of symbol `target` changed (a match's LAST byte), and bytes of later symbols too: that symbol is named,
    with reason "bytes"."""
    a, t, stores = verify_case
    block, slot = store
    ll, dd = stores[store]
    pos, lens = _positions(block, ll, dd)
    i = len(ll) - 1 if target == "last" else target
    later = [j for j in (i + 1, i + 2, i + 256, i + 1000, len(ll) - 1) if i < j < len(ll)]
    b = _flip(a, {int(pos[i] + lens[i] - 1)} | {int(pos[j]) for j in later})
    want = sc.verify_len_dist(b, *BLOCKS[block], ll, dd)
    assert want == (i, 2)                                              # the reference agrees on what was aimed at
    assert _report(gpu_ctx, t, a, b, [(block, slot, len(ll))]) == (block, i, REASON[2])


def test_kinds_of_failure(gpu_ctx, verify_case):
    """The first failing symbol as a literal, as a match whose own bytes changed, and as a match of which ONLY the
    source changed: a byte of the window before the block, which no symbol of the block stands for."""
    a, t, stores = verify_case
    seen = set()
    for store in STORES:
        block, slot = store
        ll, dd = stores[store]
        pos, lens = _positions(block, ll, dd)
        lit = next(i for i in range(300, len(ll)) if dd[i] == 0)
        mat = next(i for i in range(300, len(ll)) if dd[i] != 0)
        for kind, i, place in (("literal", lit, int(pos[lit])), ("own bytes", mat, int(pos[mat]))):
            b = _flip(a, {place, int(pos[-1])})
            assert sc.verify_len_dist(b, *BLOCKS[block], ll, dd) == (i, 2)
            assert _report(gpu_ctx, t, a, b, [(block, slot, len(ll))]) == (block, i, REASON[2])
            seen.add(kind)
        if block == 1:
            src = pos - dd.astype(np.int64)
            i = next(k for k in range(len(ll)) if dd[k] != 0 and src[k] < BLOCKS[1][0])
            b = _flip(a, {int(src[i])})
            assert b[BLOCKS[1][0]:] == a[BLOCKS[1][0]:] and dd[i] != 0
            assert sc.verify_len_dist(b, *BLOCKS[1], ll, dd) == (i, 2)
            assert _report(gpu_ctx, t, a, b, [(1, slot, len(ll))]) == (1, i, REASON[2])
            seen.add("source only")
    assert seen == {"literal", "own bytes", "source only"}


def test_first_failing_job(gpu_ctx, verify_case):
    """Several failing jobs in one call: the first failing JOB is named, in the order the call lists them; a passing job
    in front is passed over."""
    a, t, stores = verify_case
    p0, _ = _positions(0, *stores[(0, 0)])
    p1, _ = _positions(1, *stores[(1, 1)])
    n0, n1 = len(stores[(0, 0)][0]), len(stores[(1, 1)][0])
    b = _flip(a, {int(p0[500]), int(p1[90])})
    assert sc.verify_len_dist(b, *BLOCKS[0], *stores[(0, 0)]) == (500, 2)
    assert sc.verify_len_dist(b, *BLOCKS[1], *stores[(1, 1)]) == (90, 2)
    assert _report(gpu_ctx, t, a, b, [(0, 0, n0), (1, 1, n1)]) == (0, 500, REASON[2])
    assert _report(gpu_ctx, t, a, b, [(1, 1, n1), (0, 0, n0)]) == (1, 90, REASON[2])
    only1 = _flip(a, {int(p1[90])})
    assert _report(gpu_ctx, t, a, only1, [(0, 0, n0), (1, 1, n1)]) == (1, 90, REASON[2])
    assert _report(gpu_ctx, t, a, a, [(0, 0, n0), (1, 1, n1)]) is None


def test_short_stores(gpu_ctx, verify_case):
    """One symbol short and short by a whole tail: every symbol holds, they do not add up, and the report names the index
    behind the last symbol.  With a changed byte as well, the symbol comes first."""
    a, t, stores = verify_case
    ll, dd = stores[(1, 0)]
    n = len(ll)
    pos, _ = _positions(1, ll, dd)
    for short in (1, 300, n - 1, n):
        assert sc.verify_len_dist(a, *BLOCKS[1], ll[:n - short], dd[:n - short]) == (n - short, 3)
        assert _report(gpu_ctx, t, a, a, [(1, 0, n - short)]) == (1, n - short, REASON[3])
    b = _flip(a, {int(pos[100])})
    assert sc.verify_len_dist(b, *BLOCKS[1], ll[:n - 300], dd[:n - 300]) == (100, 2)
    assert _report(gpu_ctx, t, a, b, [(1, 0, n - 300)]) == (1, 100, REASON[2])


def test_error_class_of_a_failed_verification(gpu_ctx, verify_case):
    """A refusal, then a failed verification on the same thread: the class is the verification's own (ZMX_ERR_DEVICE,
    which the host layer tries again elsewhere), not the refusal's left behind; a passing call then returns 0."""
    ZMX_ERR_DEVICE, ZMX_ERR_REFUSED = 1, 3
    a, t, stores = verify_case
    ll, dd = stores[(0, 0)]
    pos, _ = _positions(0, ll, dd)
    with pytest.raises(RuntimeError, match="zmx_store_download: bad block or slot"):
        t.store(0, 2, 1)
    assert gpu_ctx.lib.zmx_last_error_class() == ZMX_ERR_REFUSED
    b = _flip(a, {int(pos[100])})
    assert sc.verify_len_dist(b, *BLOCKS[0], ll, dd) == (100, 2)
    gpu_ctx.set_input(b)
    try:
        with pytest.raises(RuntimeError) as e:
            t.verify_stores([0], [0], [len(ll)])
        cls = gpu_ctx.lib.zmx_last_error_class()
    finally:
        gpu_ctx.set_input(a)
    m = MSG.search(str(e.value))
    assert m and (int(m.group(1)), int(m.group(2)), m.group(3)) == (0, 100, REASON[2]), str(e.value)
    assert cls == ZMX_ERR_DEVICE
    t.verify_stores([0], [0], [len(ll)])                                   # passes: returns 0, raises nothing
