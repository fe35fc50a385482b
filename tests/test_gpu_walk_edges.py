"""The segmented trace (k_trace_exits / k_trace_link / k_trace_emit, zmx_trace.h) and the segmented greedy walk
(k_greedy_exits / k_greedy_link / k_greedy_emit, zmx_greedy.h) on the cases of walk_cases.py, which stand on their
edges: segment boundaries entered at every one of the 258 cells / 516 states, short last segments the walk ends above
or jumps over, restages and window edges, held matches carried into the next segment, lengths resolved through every
change point of a record.  What the cases reach is asserted without a GPU in test_cpu_walk_cases.py.

The trace runs on GIVEN length arrays (Tables.trace, zmx_trace_length_arrays: the tail of a squeeze run, the same
launches) against the Python TraceBackwards + FollowPath of walk_cases.py; the greedy against OracleTable.greedy().
Symbol counts, both store planes and histograms, integer equality, no tolerance.

The bodies take the context as an argument: test_cpu_walk_cases.py runs them against the host test library, whose
stand-in for the trace entry is a plain backward walk over the oracle's table."""
import re

import numpy as np
import pytest

import oracle_lib as ol
import steer_cases as sc
import walk_cases as wc

ZMX_ERR_DEVICE, ZMX_ERR_REFUSED = 1, 3
FLAGS = re.compile(r"zmx_trace_length_arrays: device consistency flags 0x([0-9a-f]+)$")


# ------------------------------------------------------------------------------------------------ bodies
def assert_stores(t, slots, nsym, hist, refs, what):
    for b, ref in enumerate(refs):
        assert int(nsym[b]) == len(ref["ll"]), (what, b, int(nsym[b]), len(ref["ll"]))
        ll, dd = t.store(b, int(slots[b]), nsym[b])
        assert np.array_equal(ll, ref["ll"]), (what, b, "litlens")
        assert np.array_equal(dd, ref["dd"]), (what, b, "dists")
        assert np.array_equal(hist[b], ref["hist"]), (what, b, "histogram")


def trace_object_vs_reference(ctx, key, cases=None):
    """Every case of a trace object, in its three off-path fillings, the slots changing from block to block and from
    call to call: nsym, stores and histogram of every block == the Python reference of the path."""
    o = wc.trace_object(key)
    ctx.set_input(o["data"])
    t = ctx.build_tables(o["blocks"])
    try:
        for n, case in enumerate(o["cases"] if cases is None else cases):
            refs = case.reference()
            for w, which in enumerate(wc.FILLINGS):
                slots = [(b + n + w) & 1 for b in range(len(o["blocks"]))]
                nsym, hist = t.trace(case.filled(which), slots)
                assert_stores(t, slots, nsym, hist, refs, (key, case.name, which))
    finally:
        t.free()


def _expect_flags(ctx, t, las, slots, flags):
    with pytest.raises(RuntimeError) as e:
        t.trace(las, slots)
    m = FLAGS.search(str(e.value))
    assert m and int(m.group(1), 16) == flags, str(e.value)
    assert ctx.lib.zmx_last_error_class() == ZMX_ERR_DEVICE


def _expect_refused(ctx, t, las, slots, text):
    """The refusal's whole message: the entry's name, then `text` (host/entry_checks.h holds the texts, once)."""
    with pytest.raises(RuntimeError, match="zmx_trace_length_arrays"):
        t.trace(las, slots)
    assert ctx.error() == "zmx_trace_length_arrays: " + text
    assert ctx.lib.zmx_last_error_class() == ZMX_ERR_REFUSED


def _squeeze_equals_oracle(t, o):
    """A normal squeeze run (entropy costs of the greedy parse) on tables the trace entry has written arrays into."""
    nb = len(o["blocks"])
    _, hist = t.greedy(0)
    cost, mincost = sc.cost_rows([ol.entropy_costs(h) for h in hist])
    nsym, hist = t.squeeze_run(cost, mincost, np.ones(nb, dtype=np.int32))
    for b, (s, e) in enumerate(o["blocks"]):
        tab = ol.OracleTable(o["data"], s, e)
        la, ll, dd = tab.squeeze_run(cost[b, :288], cost[b, 288:], mincost[b])
        tab.close()
        assert np.array_equal(t.length_array(b)[1:], la[1:]), b
        gl, gd = t.store(b, 1, nsym[b])
        assert np.array_equal(gl, ll) and np.array_equal(gd, dd), b
        assert np.array_equal(hist[b], wc.histogram(ll, dd)), b


def zero_on_path_reports(ctx):
    """A 0 on the path — at the top cell, inside a segment, at a segment's entry cell, at cell 1 — is reported as flag
    0x2 (on zeros every length is valid: nothing else can fire); a correct call on the same tables follows each."""
    o = wc.trace_object("zero_edges")
    case = o["cases"][5]
    refs = case.reference()
    nb = len(o["blocks"])
    slots = [b & 1 for b in range(nb)]
    ctx.set_input(o["data"])
    t = ctx.build_tables(o["blocks"])
    try:
        good = case.filled("zeros")
        for b, pick in ((1, "top"), (1, "middle"), (0, "entry"), (6, "entry"), (2, "last"), (6, "middle")):
            heads = refs[b]["heads"]
            segs = wc.trace_segments(good[b], heads)
            if pick == "top":
                h = heads[0]
            elif pick == "last":
                h = heads[-1]
            elif pick == "entry":
                seg = segs[1]
                h = len(good[b]) - 1 - seg["s"] * wc.TS_SEG - seg["j"]
                assert h in heads and not seg["skipped"]
            else:
                h = heads[len(heads) // 2]
            las = [a.copy() for a in good]
            las[b][h] = 0
            with pytest.raises(wc.ZeroOnPath):
                wc.walk_back(las[b])
            _expect_flags(ctx, t, las, slots, 0x2)
            nsym, hist = t.trace(good, slots)
            assert_stores(t, slots, nsym, hist, refs, ("after a zero on the path", b, pick))
        _squeeze_equals_oracle(t, o)
    finally:
        t.free()


def refusals(ctx):
    """What the host refuses before any launch: a cell at 259, at 2, above its own index; a wrong number of blocks or
    cells; a slot that is none; trimmed and matches-only tables.  Class REFUSED; a correct call follows each."""
    o = wc.trace_object("zero_edges")
    case = o["cases"][8]
    refs = case.reference()
    nb = len(o["blocks"])
    slots = [1 - (b & 1) for b in range(nb)]
    ctx.set_input(o["data"])
    t = ctx.build_tables(o["blocks"])
    try:
        good = case.filled("range")

        def bad(b, h, v):
            las = [a.copy() for a in good]
            las[b][h] = v
            return las, f"block {b}, cell {h} holds {v}: no step of a path"

        off_path = next(h for h in range(3000, 4000) if case.las[1][h] == 0)
        on_path = refs[1]["heads"][7]
        for las, text in (bad(1, off_path, 259), bad(1, on_path, 259), bad(1, off_path, 2), bad(1, on_path, 2), bad(0, 0, 1),
                          bad(0, 1, 3), bad(2, 5, 6), bad(6, 100, 101), bad(nb - 1, len(good[nb - 1]) - 1, 65535)):
            _expect_refused(ctx, t, las, slots, text)
            nsym, hist = t.trace(good, slots)
            assert_stores(t, slots, nsym, hist, refs, "after a refusal")
        per_block = "one length array per block of the tables"
        size0 = len(good[0]) - 1
        _expect_refused(ctx, t, good[:-1], slots[:-1], per_block)                     # a block short
        _expect_refused(ctx, t, good + [good[0]], slots + [0], per_block)             # a block too many
        _expect_refused(ctx, t, [good[0][:-1]] + good[1:], slots,                     # a cell short
                        f"block 0 has {size0} + 1 cells, not {size0}")
        _expect_refused(ctx, t, [np.append(good[0], 1)] + good[1:], slots, f"block 0 has {size0} + 1 cells, not {size0 + 2}")
        _expect_refused(ctx, t, good, [2] + slots[1:], "slot must be 0 or 1")
        # the valid side of the rule: 0 anywhere off the path, 1 at cell 1, 258 at cell 258, h at cell h < 258
        las = [a.copy() for a in case.las]
        for b in range(nb):
            for h, v in ((1, 1), (3, 3), (257, 257), (258, 258), (259, 258)):
                if case.las[b][h] == 0:
                    las[b][h] = v
        nsym, hist = t.trace(las, slots)
        assert_stores(t, slots, nsym, hist, refs, "valid edges")
        t.trim()
        _expect_refused(ctx, t, good, slots, "these tables were trimmed to their stores (zmx_tables_trim)")
    finally:
        t.free()
    t = ctx.build_tables(o["blocks"], matches_only=True)
    try:
        _expect_refused(ctx, t, good, slots, "these tables hold matches only (zmx_tables_build_matches)")
    finally:
        t.free()


def missing_length_reports(ctx, key):
    """A length of the valid range that the record at the symbol's start does not hold — one above its longest, at a
    position without a match, with an inline record, with a pool record — is reported as flag 0x4; a correct call on
    the same tables follows each, and a normal squeeze run after them equals the oracle's."""
    o = wc.trace_object(key)
    case = o["cases"][0]
    refs = case.reference()
    ctx.set_input(o["data"])
    t = ctx.build_tables(o["blocks"])
    try:
        arrays = wc.missing_length_arrays(key)
        assert arrays
        for what, p, step, la in arrays:
            with pytest.raises(wc.MissingLength):
                wc.trace_reference(o["data"], o["blocks"][0][0], la, o["resolve"][0])
            _expect_flags(ctx, t, [la], [1], 0x4)
            nsym, hist = t.trace(case.filled("path"), [0])
            assert_stores(t, [0], nsym, hist, refs, ("after a missing length", what))
        _squeeze_equals_oracle(t, o)
    finally:
        t.free()


def greedy_vs_reference(ctx, data, blocks, refs, matches_only, slot=0):
    ctx.set_input(data)
    t = ctx.build_tables(blocks, matches_only=matches_only)
    try:
        nsym, hist = t.greedy(slot)
        assert_stores(t, [slot] * len(blocks), nsym, hist, refs, "greedy")
    finally:
        t.free()


@pytest.fixture(scope="module")
def class_refs():
    """OracleTable.greedy() with its histogram for the class data cut into the edge-size blocks."""
    out = {}
    for cls in wc.CLASS_BLOCKS:
        c = wc.class_blocks(cls)
        refs = []
        for s, e in c["blocks"]:
            tab = ol.OracleTable(c["data"], s, e)
            ll, dd = tab.greedy()
            tab.close()
            refs.append(dict(ll=ll, dd=dd, hist=ol.histogram(ll, dd)))
        out[cls] = refs
    return out


# ------------------------------------------------------------------------------------------------ GPU tests
@pytest.mark.gpu
def test_trace_constant_steps_over_edge_sizes(gpu_ctx):
    """Steps of 1, 3, 4, 64, 129, 257 and 258 over blocks of every edge size (and an empty one between two others) in
    one call each."""
    trace_object_vs_reference(gpu_ctx, "zero_sizes")


ENTRY_GROUPS = 6


@pytest.mark.gpu
@pytest.mark.parametrize("group", range(ENTRY_GROUPS))
def test_trace_entry_offsets(gpu_ctx, group):
    """A step that lands j cells below the top of the lower segment, j = 0 .. 257, at full and at short segments, and
    the walks that end exactly at cell 0 above a bottom segment of 1, 2, 3 or 257 cells."""
    cases = wc.trace_object("zero_edges")["cases"]
    per = (len(cases) + ENTRY_GROUPS - 1) // ENTRY_GROUPS
    trace_object_vs_reference(gpu_ctx, "zero_edges", cases[group * per:(group + 1) * per])


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(wc.REAL))
def test_trace_random_paths_on_real_records(gpu_ctx, key):
    trace_object_vs_reference(gpu_ctx, key)


@pytest.mark.gpu
def test_trace_reports_a_zero_on_the_path(gpu_ctx):
    zero_on_path_reports(gpu_ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["M", "prefix8"])
def test_trace_reports_a_missing_length(gpu_ctx, key):
    missing_length_reports(gpu_ctx, key)


@pytest.mark.gpu
def test_trace_refusals(gpu_ctx):
    refusals(gpu_ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("matches_only", [False, True], ids=["full", "matches"])
@pytest.mark.parametrize("group", range(wc.PLANTED_GROUPS))
def test_greedy_planted_entry_states(gpu_ctx, group, matches_only):
    """Planted copies that end j positions into the second segment (j = 0 .. 257), a match held across the segment
    start in both outcomes, a top segment jumped over."""
    g = wc.planted_group(group)
    greedy_vs_reference(gpu_ctx, g["data"], g["blocks"], g["refs"], matches_only, slot=group & 1)


@pytest.mark.gpu
@pytest.mark.parametrize("matches_only", [False, True], ids=["full", "matches"])
@pytest.mark.parametrize("cls", wc.CLASS_BLOCKS)
def test_greedy_edge_size_blocks(gpu_ctx, class_refs, cls, matches_only):
    c = wc.class_blocks(cls)
    greedy_vs_reference(gpu_ctx, c["data"], c["blocks"], class_refs[cls], matches_only)
