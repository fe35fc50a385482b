"""What the zmx_* entries refuse before they touch anything (the rules of csrc/host/entry_checks.h): a block, a slot
or a symbol count that the tables do not have, trimmed tables, tables that hold matches only.  Every refusal is class
ZMX_ERR_REFUSED and its message is the entry's own name, then the one text all entries share.  String and integer
equality, no tolerance.

The case: class M, 7 000 bytes, blocks [(0, 3000), (3000, 7000)], a greedy store in slot 0 and one squeeze run in slot
1.  "One symbol too many" is asked of the squeeze run's stores: those end at the block's end, so the layer knows their
count.  A greedy store starts at the front of its slot and the layer does not keep its count; there the bound is the
block's size, and one more than that is refused.

The bodies take the context as an argument: test_cpu_entry_checks.py runs them against the host test library, whose
stand-in for the device layer calls the same rules."""
import ctypes

import numpy as np
import pytest

import oracle_lib as ol
import steer_cases as sc
from zopfli_amd import generate
from zopfli_amd.api import CostStores

ZMX_ERR_DEVICE, ZMX_ERR_REFUSED = 1, 3
BLOCKS = [(0, 3000), (3000, 7000)]
TRIMMED = "these tables were trimmed to their stores (zmx_tables_trim)"
MATCHES_ONLY = "these tables hold matches only (zmx_tables_build_matches)"
CODES = sc.codes_15bit(5)


# ------------------------------------------------------------------------------------------------ bodies
def _download_batch(t, block, slot, nsym):
    """zmx_store_download_batch of one store."""
    ll = np.zeros(max(int(nsym), 1), dtype=np.uint16)
    dd = np.zeros(max(int(nsym), 1), dtype=np.uint16)
    fn = t.ctx.lib.zmx_store_download_batch
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t] + [ctypes.c_void_p] * 5
    b, s, k = (ctypes.c_size_t * 1)(block), (ctypes.c_int32 * 1)(slot), (ctypes.c_size_t * 1)(int(nsym))
    pl, pd = (ctypes.c_void_p * 1)(ll.ctypes.data), (ctypes.c_void_p * 1)(dd.ctypes.data)
    t.ctx._check(fn(t.ctx.handle, t.handle, 1, ctypes.cast(b, ctypes.c_void_p), ctypes.cast(s, ctypes.c_void_p),
                    ctypes.cast(k, ctypes.c_void_p), ctypes.cast(pl, ctypes.c_void_p), ctypes.cast(pd, ctypes.c_void_p)),
                 "zmx_store_download_batch")
    return ll[:int(nsym)], dd[:int(nsym)]


def _cost_stores(t, block, slot, nsym):
    CostStores.from_tables(t, [[(block, slot, nsym)]]).free()


# the five entries that name a store: name of the C entry -> call(t, block, slot, nsym, nbits)
STORE_ENTRIES = {
    "zmx_store_download": lambda t, b, s, k, bits: t.store(b, s, k),
    "zmx_store_download_batch": lambda t, b, s, k, bits: _download_batch(t, b, s, k),
    "zmx_verify_stores": lambda t, b, s, k, bits: t.verify_stores([b], [s], [k]),
    "zmx_encode_blocks": lambda t, b, s, k, bits: t.encode_blocks([(b, s, k, 0, bits)], CODES),
    "zmx_cost_stores_create": lambda t, b, s, k, bits: _cost_stores(t, b, s, k),
}


def _refused(ctx, call, message):
    with pytest.raises(RuntimeError):
        call()
    assert ctx.error() == message
    assert ctx.lib.zmx_last_error_class() == ZMX_ERR_REFUSED, message


def entry_case(ctx, matches_only=False):
    """(Tables, {slot: nsym per block}, (cost, mincost)): the greedy parse in slot 0 and, on full tables, a run in slot 1."""
    ctx.set_input(generate("M", BLOCKS[-1][1]))
    t = ctx.build_tables(BLOCKS, matches_only=matches_only)
    nsym0, hist = t.greedy(0)
    model = sc.cost_rows([ol.entropy_costs(h) for h in hist])
    counts = {0: nsym0}
    if not matches_only:
        counts[1], _ = t.squeeze_run(*model, np.ones(len(BLOCKS), dtype=np.int32))
    return t, counts, model


def store_refs_checked(ctx):
    """Every store entry: block = nb, slot 2 and -1, one symbol too many are refused; the store's count and 0 are not."""
    t, counts, _ = entry_case(ctx)
    nb = len(BLOCKS)
    try:
        for who, call in STORE_ENTRIES.items():
            for block, slot, nsym in ((nb, 0, 1), (0, 2, 1), (1, -1, 1)):
                _refused(ctx, lambda: call(t, block, slot, nsym, 15), who + ": bad block or slot")
            for b in range(nb):
                size = BLOCKS[b][1] - BLOCKS[b][0]
                _refused(ctx, lambda: call(t, b, 1, int(counts[1][b]) + 1, 15), who + ": nsym exceeds the store")
                _refused(ctx, lambda: call(t, b, 0, size + 1, 15), who + ": nsym exceeds the store")
            for b in range(nb):
                for slot in (0, 1):
                    n = int(counts[slot][b])
                    ll, dd = t.store(b, slot, n)
                    assert len(ll) == n and n > 0
                    call(t, b, slot, n, int(sc.symbol_bits(ll, dd, CODES).sum()) + 15)
                    if who == "zmx_verify_stores":
                        # no symbols do not add up to a block: the check lets the call through and the DEVICE says so
                        with pytest.raises(RuntimeError):
                            call(t, b, slot, 0, 15)
                        assert ctx.lib.zmx_last_error_class() == ZMX_ERR_DEVICE, ctx.error()
                    else:
                        call(t, b, slot, 0, 15)
    finally:
        t.free()


def trimmed_tables_refuse(ctx, hash_links=True, dp_rows=True):
    """After zmx_tables_trim the stores are still served; everything that needs more says so."""
    t, counts, model = entry_case(ctx)
    try:
        t.trim()
        las = [np.zeros(e - s + 1, dtype=np.uint16) for s, e in BLOCKS]
        calls = {
            "zmx_verify_stores": lambda: t.verify_stores([0], [0], [int(counts[0][0])]),
            "zmx_squeeze_run": lambda: t.squeeze_run(*model, [1, 1]),
            "zmx_lz77_greedy": lambda: t.greedy(0),
            "zmx_trace_length_arrays": lambda: t.trace(las, [0, 0]),
            "zmx_find_longest_match": lambda: t.find_longest_match(0, 10),
            "zmx_length_array_download": lambda: t.length_array(0),
        }
        if hash_links:
            calls["zmx_hash_links_download"] = lambda: t.hash_links(0)
        if dp_rows:
            calls["zmx_dp_rows_download"] = lambda: t.dp_rows(0)
            calls["zmx_chain_tasks_download"] = lambda: t.chain_tasks()
        for who, call in calls.items():
            _refused(ctx, call, f"{who}: {TRIMMED}")
        for b in range(len(BLOCKS)):
            assert len(t.store(b, 1, counts[1][b])[0]) == counts[1][b]
    finally:
        t.free()


def matches_only_tables_refuse(ctx, dp_rows=True):
    t, counts, model = entry_case(ctx, matches_only=True)
    try:
        las = [np.zeros(e - s + 1, dtype=np.uint16) for s, e in BLOCKS]
        _refused(ctx, lambda: t.squeeze_run(*model, [1, 1]), f"zmx_squeeze_run: {MATCHES_ONLY}")
        _refused(ctx, lambda: t.trace(las, [0, 0]), f"zmx_trace_length_arrays: {MATCHES_ONLY}")
        if dp_rows:
            _refused(ctx, lambda: t.dp_rows(0), f"zmx_dp_rows_download: {MATCHES_ONLY}")
            _refused(ctx, lambda: t.chain_tasks(), f"zmx_chain_tasks_download: {MATCHES_ONLY}")
        assert np.array_equal(t.greedy(1)[0], counts[0])
    finally:
        t.free()


def probe_blocks_checked(ctx):
    """The probes that name a block alone: block = nb is refused, the last block is served."""
    t, _, _ = entry_case(ctx)
    try:
        nb = len(BLOCKS)
        _refused(ctx, lambda: t.dp_rows(nb), "zmx_dp_rows_download: bad block")
        assert len(t.dp_rows(nb - 1)["kend"]) == BLOCKS[-1][1] - BLOCKS[-1][0]
        # zmx_chain_tasks_download names no block; its sizes-first call: the arrays have the sizes it reported, every
        # block has a first task, and the tasks are those of the two lists
        ct = t.chain_tasks()
        nt = len(ct["tasks"])
        assert nt >= nb and len(ct["task_off"]) == nb + 1 and int(ct["task_off"][-1]) == nt
        assert len(ct["wg_desc"]) == ct["n_wg"] + ct["n_wg_runs"] > 0
        assert sorted(map(int, ct["wg_tasks"])) == list(range(nt)) and int(ct["wg_desc"][:, 1].sum()) == nt
        assert [int(ct["tasks"][int(k), 2]) for k in ct["task_off"][:-1]] == [0] * nb
    finally:
        t.free()


# ------------------------------------------------------------------------------------------------ on the device
@pytest.mark.gpu
def test_store_refs_checked(gpu_ctx):
    store_refs_checked(gpu_ctx)


@pytest.mark.gpu
def test_trimmed_tables_refuse(gpu_ctx):
    trimmed_tables_refuse(gpu_ctx)


@pytest.mark.gpu
def test_matches_only_tables_refuse(gpu_ctx):
    matches_only_tables_refuse(gpu_ctx)


@pytest.mark.gpu
def test_probe_blocks_checked(gpu_ctx):
    probe_blocks_checked(gpu_ctx)


@pytest.mark.gpu
def test_store_download_paths_agree(gpu_ctx):
    """zmx_store_download and zmx_store_download_batch split a store's u32 symbols with one function (UnpackSymbols,
    drv_stores.h) behind their own copy paths.  8 KiB of class T, one block, the greedy parse in slot 0: both entries
    return the same litlens and dists, and those are the CPU oracle's greedy store.  Integer equality."""
    data = generate("T", 8192)
    gpu_ctx.set_input(data)
    t = gpu_ctx.build_tables([(0, len(data))])
    try:
        nsym = int(t.greedy(0)[0][0])
        want = ol.OracleTable(data, 0, len(data)).greedy()
        assert nsym == len(want[0]) > 0
        one = t.store(0, 0, nsym)
        many = _download_batch(t, 0, 0, nsym)
        for got in (one, many):
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert np.array_equal(one[0], many[0]) and np.array_equal(one[1], many[1])
    finally:
        t.free()
