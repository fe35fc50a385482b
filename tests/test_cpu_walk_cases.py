"""What the cases of walk_cases.py reach, asserted with the plain references alone: test_gpu_walk_edges.py holds the
trace and greedy kernels to the same references, so a generator that quietly covered less would fail HERE, without a
GPU.  Also: the refusal rules of zmx_trace_length_arrays and the host test library's stand-in for it, by running the
GPU file's own bodies against that library.  CPU only."""
import numpy as np
import pytest

import oracle_lib as ol
import walk_cases as wc

ZMX_ERR_REFUSED = 3


# ------------------------------------------------------------------------------------------------ the references
def test_zeros_have_one_distance():
    assert wc.zeros_distance() == 1


@pytest.mark.parametrize("key", wc.TRACE_OBJECTS)
def test_fillings_leave_the_path_alone(key):
    """Zeros, other valid values or a second path in the off-path cells: the same walk, the same symbols; the second
    path IS a different one, and both are valid (every length is held by the record at its start)."""
    o = wc.trace_object(key)
    for case in o["cases"]:
        refs = case.reference()
        f = {w: case.filled(w) for w in wc.FILLINGS}
        for b, (s, e) in enumerate(o["blocks"]):
            assert len(case.las[b]) == e - s + 1
            for w in wc.FILLINGS:
                la = f[w][b]
                assert la[0] == 0 and np.all(la != 2) and np.all(la <= np.minimum(np.arange(len(la)), 258))
                assert wc.walk_back(la) == refs[b]["heads"], (key, case.name, b, w)
            off = int(np.count_nonzero(case.las[b][1:] == 0))
            if e - s > 600 and off > 300:
                other = wc.trace_reference(o["data"], s, case.others[b], o["resolve"][b])
                assert other["heads"] != refs[b]["heads"]
                assert np.count_nonzero(f["path"][b] != f["zeros"][b]) > 0
                assert np.count_nonzero(f["range"][b] != f["zeros"][b]) == off


@pytest.mark.parametrize("key", list(wc.REAL))
def test_python_trace_equals_the_oracle_on_its_own_array(key):
    """trace_reference on the length array of an oracle squeeze run == the oracle's TraceBackwards + FollowPath."""
    o = wc.trace_object(key)
    s, e = o["blocks"][0]
    tab = ol.OracleTable(o["data"], s, e)
    ll_o, dd_o = tab.greedy()
    costs = ol.entropy_costs(ol.histogram(ll_o, dd_o))
    la, ll, dd = tab.squeeze_run(costs[0], costs[1], ol.model_min_cost(*costs))
    tab.close()
    ref = wc.trace_reference(o["data"], s, la, o["resolve"][0])
    assert np.array_equal(ref["ll"], ll) and np.array_equal(ref["dd"], dd)
    assert np.array_equal(ref["hist"], ol.histogram(ll, dd))


# ------------------------------------------------------------------------------------------------ what the trace cases reach
@pytest.fixture(scope="module")
def trace_reach():
    """Every (object, case, block): its segments (trace_segments) and the change points its symbols resolve through."""
    out = []
    for key in wc.TRACE_OBJECTS:
        o = wc.trace_object(key)
        for case in o["cases"]:
            for b, ref in enumerate(case.reference()):
                out.append((key, case.name, b, ref, wc.trace_segments(case.las[b], ref["heads"])))
    return out


def test_all_entry_offsets_occur_at_a_boundary(trace_reach):
    full, short = set(), set()
    for key, name, b, ref, segs in trace_reach:
        for g in segs[1:]:
            if not g["skipped"]:
                (full if g["cells"] == wc.TS_SEG else short).add(g["j"])
    assert full == set(range(wc.TS_ENT))                                   # into a segment of 4096 cells
    assert short >= set(range(wc.TS_ENT))                                  # and into a short last one (259 cells)


def test_walk_ends_above_every_short_segment(trace_reach):
    """... exactly at cell 0, from the segment above, for a bottom segment of 1, 2, 3 and 257 cells — and enters the
    same segments in other cases."""
    skipped, entered = set(), set()
    for key, name, b, ref, segs in trace_reach:
        for g in segs[1:]:
            (skipped if g["skipped"] else entered).add(g["cells"])
            if g["skipped"]:
                assert g["j"] == g["cells"] and g["nsym"] == 0 and g is segs[-1]
    assert skipped >= set(wc.SHORT_R)
    assert entered >= set(wc.SHORT_R)


def test_symbol_lengths_and_block_sizes(trace_reach):
    lengths, sizes = set(), set()
    for key, name, b, ref, segs in trace_reach:
        lengths |= set(ref["ll"][ref["dd"] != 0].tolist())
        if key == "zero_sizes":
            sizes.add(len(ref["heads"]) and ref["heads"][0])
    assert {3, 4, 64, 129, 257, 258} <= lengths
    assert sizes == set(wc.EDGE_SIZES) | {0}
    real = set()
    for key, name, b, ref, segs in trace_reach:
        if key in wc.REAL:
            real |= set(ref["ll"][ref["dd"] != 0].tolist())
    assert 3 in real and 258 in real and len(real) > 200


def test_change_points_resolved_through(trace_reach):
    """Every inline change-point index 0 .. 7 resolves a path symbol (records of up to 8 change points), for the last
    of them at index 7 of a record of exactly 8; records of more than 8 (the pool's binary search) resolve 50 or more,
    at their first, their last and inner entries."""
    inline, pool, pool_where = set(), 0, set()
    for key, name, b, ref, segs in trace_reach:
        for k, ncp in ref["via"]:
            if ncp <= 8:
                inline.add((k, ncp))
            else:
                pool += 1
                pool_where.add("first" if k == 0 else "last" if k == ncp - 1 else "inner")
    print("inline (index, change points):", sorted(inline), "pool symbols:", pool)
    assert {k for k, _ in inline} == set(range(8))
    assert (7, 8) in inline and (0, 1) in inline
    assert pool >= 50
    assert pool_where == {"first", "last", "inner"}


def test_restages_and_batches(trace_reach):
    """Path heads on both sides of a restage of k_trace_emit's 2048 staged cells; segments of more than 64 symbols (a
    second resolve batch), of exactly 64 and 65 and 1, and segments that emit none."""
    restages, nsyms = set(), set()
    for key, name, b, ref, segs in trace_reach:
        for g in segs:
            restages.add(g["restages"])
            nsyms.add(g["nsym"])
    assert {1, 2, 3} <= restages
    assert 0 in nsyms and 1 in nsyms and max(nsyms) == wc.TS_SEG
    assert {63, 64, 65} <= nsyms and any(64 < n < 128 for n in nsyms) and any(n > 128 for n in nsyms)


def test_missing_length_arrays_are_what_they_claim():
    found = set()
    for key in ("M", "prefix8"):
        o = wc.trace_object(key)
        rec = o["records"]
        for what, p, step, la in wc.missing_length_arrays(key):
            found.add(what)
            assert la[p + step] == step and 3 <= step <= 258
            assert np.all(la != 2) and np.all(la <= np.minimum(np.arange(len(la)), 258))      # the host accepts it
            assert rec.resolve(p, step)[0] == 0 and (step == 3 or rec.resolve(p, step - 1)[0] != 0)
            with pytest.raises(wc.MissingLength) as e:
                wc.trace_reference(o["data"], o["blocks"][0][0], la, rec.resolve)
            assert e.value.args[0] == (p, step)                                                 # the only one on the path
    assert found == {"none", "inline", "pool"}


# ------------------------------------------------------------------------------------------------ the greedy cases
def test_lazy_automaton_equals_the_oracle():
    """The Python automaton over the oracle's records == OracleTable.greedy(), symbol for symbol, on the class data cut
    into the edge sizes and on every planted block."""
    for cls in wc.CLASS_BLOCKS:
        c = wc.class_blocks(cls)
        for s, e in c["blocks"]:
            rec = wc.Records(c["data"], s, e)
            ll, dd, visited, _ = wc.lazy_automaton(c["data"], s, rec.length, rec.dist)
            tab = ol.OracleTable(c["data"], s, e)
            oll, odd = tab.greedy()
            tab.close()
            assert np.array_equal(ll, oll) and np.array_equal(dd, odd), (cls, s, e)
            assert np.array_equal(wc.histogram(ll, dd), ol.histogram(oll, odd))
    for g in range(wc.PLANTED_GROUPS):
        grp = wc.planted_group(g)
        for (s, e), ref in zip(grp["blocks"], grp["refs"]):
            tab = ol.OracleTable(grp["data"], s, e)
            oll, odd = tab.greedy()
            tab.close()
            assert np.array_equal(ref["ll"], oll) and np.array_equal(ref["dd"], odd), (g, s, e)
            assert np.array_equal(ref["hist"], ol.histogram(oll, odd))


def test_greedy_entry_states_reached():
    """All 258 (j, 0) entry states (j = 256 and 257 are the second pass of the 512 threads over the 516 states), the
    held state (0, 1) with both outcomes, and a top segment of 1, 2, 3 and 257 positions jumped over."""
    plain, held, jumped = set(), set(), set()
    for g in range(wc.PLANTED_GROUPS):
        grp = wc.planted_group(g)
        assert len(grp["data"]) <= 100000
        for (kind, arg), ref in zip(grp["specs"], grp["refs"]):
            (entry,) = ref["entries"]
            if entry[0] == "jumped":
                jumped.add(entry[1])
                assert ref["dd"][-1] != 0                                  # the last symbol is the match that jumps
            elif entry[1]:
                assert entry[0] == 0
                held.add(ref["held"][wc.TS_SEG])
            else:
                plain.add(entry[0])
    assert plain == set(range(wc.TS_ENT))
    assert held == {"match", "literal"}
    assert jumped == set(wc.SHORT_R)


# ------------------------------------------------------------------------------------------------ hook and stand-in
@pytest.fixture(scope="module")
def host_ctx():
    from zopfli_amd import Context
    ctx = Context(0, ol.hosttest_library())
    yield ctx
    ctx.close()


def test_refusal_rules_host_backend(host_ctx):
    from test_gpu_walk_edges import refusals
    refusals(host_ctx)


def test_cell_rule_at_its_edges(host_ctx):
    """The cell rule of zmx_trace_length_arrays (PathCell, csrc/host/entry_checks.h: the device layer and the host test
    library run the same function) at cells 0, 1, 2, 3, 257, 258, 259 and 300 of one block of 300 bytes, each holding 0,
    1, 2, 3, h - 1, h, h + 1, 258 and 259 in turn.  A cell is accepted exactly when its value is 0 or 1 or a length
    3 .. min(h, 258) — and no step back past the block's start: a 1 in cell 0 is refused, as it was before the rule had
    a home of its own (refusals() of test_gpu_walk_edges.py asserts that one case on the device as well).  A refusal
    carries the full text and class REFUSED; an accepted array is traced, or fails for what its path holds (class
    DEVICE) — never as a refusal."""
    from zopfli_amd import generate
    size = 300
    host_ctx.set_input(generate("M", size))
    t = host_ctx.build_tables([(0, size)])
    try:
        base = np.ones(size + 1, dtype=np.uint16)       # a path of literals: valid, and every cell is on it
        base[0] = 0
        tried = 0
        for h in (0, 1, 2, 3, 257, 258, 259, 300):
            for v in sorted({0, 1, 2, 3, h - 1, h, h + 1, 258, 259}):
                if v < 0:
                    continue
                la = base.copy()
                la[h] = v
                accept = (v in (0, 1) or 3 <= v <= min(h, 258)) and v <= h
                try:
                    t.trace([la], [0])
                    refused = False
                except RuntimeError:
                    refused = host_ctx.lib.zmx_last_error_class() == ZMX_ERR_REFUSED
                assert refused == (not accept), (h, v)
                if refused:
                    assert host_ctx.error() == f"zmx_trace_length_arrays: block 0, cell {h} holds {v}: no step of a path"
                tried += 1
        assert tried == 56                              # (72 pairs less h - 1 = -1 and the values that coincide)
    finally:
        t.free()


def test_error_reports_host_backend(host_ctx):
    from test_gpu_walk_edges import missing_length_reports, zero_on_path_reports
    zero_on_path_reports(host_ctx)
    missing_length_reports(host_ctx, "M")


@pytest.mark.parametrize("key", wc.TRACE_OBJECTS)
def test_stand_in_equals_the_python_trace(host_ctx, key):
    from test_gpu_walk_edges import trace_object_vs_reference
    trace_object_vs_reference(host_ctx, key)


def test_greedy_bodies_run_on_the_host_backend(host_ctx):
    from test_gpu_walk_edges import greedy_vs_reference
    g = wc.planted_group(11)
    greedy_vs_reference(host_ctx, g["data"], g["blocks"], g["refs"], False)
    greedy_vs_reference(host_ctx, g["data"], g["blocks"], g["refs"], True, slot=1)
