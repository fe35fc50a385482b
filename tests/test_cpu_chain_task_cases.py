"""chain_task_cases.py without a device: every case is held to the edge it was glued to stand on — computed from the
reference alone, so that a later change to a builder cannot quietly stop reaching it, and test_gpu_chain_tasks.py then
runs exactly these cases — and the reference's cut points are held to the definition, position by position.  For every
deliberately wrong variant of the reference (chain_task_cases.MUTANTS) a named case tells it from the right one: a
device that made that mistake would differ from the reference there.  Integer equality throughout."""
import pytest

import chain_task_cases as cc


def _block(data, name):
    d = cc.data(data)
    b = d.names[name]
    return b, d.sizes[b], cc.layouts(data)[b]


def _split_task(case, name, pout):
    """[q, pout, pend, found, wide] of the block's task `pout` before the merge."""
    b, _, _ = _block(cc.CASES[case][0], name)
    (row,) = [r for r in cc.reference(case)["split"][b] if r[1] == pout]
    return row


def _kept(case, name):
    """[q, pout, pend, kind, g, windows] of the block's tasks after the merge."""
    ref = cc.reference(case)
    b, _, _ = _block(cc.CASES[case][0], name)
    return [list(map(int, ref["tasks"][k][1:])) + [int(ref["kind"][k]), ref["g"][k], ref["windows"][k]]
            for k in range(int(ref["task_off"][b]), int(ref["task_off"][b + 1]))]


def _kept_task(case, name, pout):
    (row,) = [r for r in _kept(case, name) if r[1] == pout]
    return row


def _lane(case, q, pout):
    k = cc.knobs(case)
    at = q - 1 - cc.scan_start(pout, k["cuts"], cc.knob_warm(k["warm"]))
    return at // 64, at % 64


# ------------------------------------------------------------------------------------------------ the reference itself
def test_cut_points_by_the_definition():
    """One small block (600 positions: a literal, a copy, random bytes) and one with runs (1 100): for every q, loop
    over all p < q."""
    for data, name in (("cuts", "q1"), ("cuts", "head_wide")):
        _, B, lay = _block(data, name)
        is_cut = cc.cut_points(lay["kend"])
        assert len(is_cut) == B + 1 and not is_cut[0]
        for q in range(1, B + 1):
            assert bool(is_cut[q]) == all(p + int(lay["kend"][p]) <= q for p in range(q)), q


@pytest.mark.parametrize("case", list(cc.CASES))
def test_windowed_scan_equals_the_definition(case):
    """The scan in 64-position chunks from 258 before the lowest admissible q (or from the start of a longer warm-up
    stretch) finds, with its carry, what the definition over the whole block gives: for every task of every case."""
    name = cc.CASES[case][0]
    k = cc.knobs(case)
    n = 0
    for lay, rows in zip(cc.layouts(name), cc.reference(case)["split"]):
        for q, pout, _, found, _ in rows:
            if pout and k["cuts"]:
                assert cc.windowed_last_cut(lay["kend"], pout, k["cuts"], cc.knob_warm(k["warm"])) == (q if found else None), pout
                n += 1
    assert n > 0 or k["cuts"] == 0


@pytest.mark.parametrize("case", list(cc.CASES))
def test_reference_keeps_the_invariants(case):
    name = cc.CASES[case][0]
    assert cc.invariants(cc.reference(case), cc.data(name).sizes, cc.layouts(name), cc.knobs(case)) is None
    assert len(cc.data(name).data) <= 65536


def test_materials():
    """Random bytes: a cut point at almost every position; a copy: none strictly inside, one at either end; a run: its
    rows have 64 edges and more up to 64 bytes before its end, shortcut flags only where it is longer than 516."""
    _, _, lay = _block("cuts", "lanes")                 # random to 1087, a copy to 2090
    is_cut = cc.cut_points(lay["kend"])
    assert is_cut[1:1088].sum() >= 1080 and not is_cut[1088:2090].any() and is_cut[1087] and is_cut[2090]
    _, _, lay = _block("cuts", "wide3")                 # a run in [200, 2200)
    wide = (lay["run_row"] != 0) & (lay["kend"] >= 64)
    assert wide[201:2200 - 63].all() and not wide[2200 - 63:].any() and not wide[:201].any()
    assert lay["shortcut"].any() and not cc.cut_points(lay["kend"])[202:2200].any()
    _, _, lay = _block("cuts", "cut_behind")            # a run of 451 bytes
    assert not lay["shortcut"].any() and ((lay["run_row"] != 0) & (lay["kend"] >= 64)).any()


# ------------------------------------------------------------------------------------------------ k_cutpoints
def test_chosen_cut_on_lane_0_lane_63_and_in_the_partial_chunk():
    q, pout, _, found, _ = _split_task("cuts", "lanes", 2048)
    assert found and _lane("cuts", q, pout)[1] == 0 and pout > 1024 + 258
    q, pout, _, found, _ = _split_task("cuts", "lanes", 3072)
    assert found and _lane("cuts", q, pout)[1] == 63 and pout > 1024 + 258
    q, pout, _, found, _ = _split_task("cuts", "lanes", 2304)
    start = cc.scan_start(pout, 1024, 512)
    assert found and q == pout - 1 and (pout - start) % 64 != 0 and _lane("cuts", q, pout)[0] == (pout - 1 - start) // 64


def test_carry_over_whole_chunks():
    """Task 2048 of "carry": the match of 200 at 1720 begins in one chunk of the scan, covers three whole ones and ends
    two positions into the next; the copy that begins on its last byte hides the cut point behind it.  Without the
    carry position 1919 (lane 0 of that chunk) looks like a cut point; with it the task takes 1720.  Task 2304 takes the
    cut point behind both, 2100."""
    _, _, lay = _block("cuts", "carry")
    q, pout, _, found, _ = _split_task("cuts", "carry", 2048)
    assert found and q == 1720 and int(lay["kend"][1720]) == 200
    assert cc.windowed_last_cut(lay["kend"], pout, 1024, 512, carry=False) == 1919
    assert _lane("cuts", 1919, pout)[1] == 0 and _lane("cuts", 1919, pout)[0] - _lane("cuts", 1721, pout)[0] == 4
    assert not cc.cut_points(lay["kend"])[1721:2100].any()
    assert _split_task("cuts", "carry", 2304)[0] == 2100


def test_search_range_ends():
    is_cut = lambda name: cc.cut_points(_block("cuts", name)[2]["kend"])      # noqa: E731
    # exactly pout - depth: taken
    q, pout, _, found, _ = _split_task("cuts", "exact_depth", 2048)
    assert found and q == pout - 1024 and pout > 1024 + 258 and not is_cut("exact_depth")[q + 1:pout].any()
    # pout - depth - 1 and nothing above: none, the task keeps its warm-up start and is not wide
    q, pout, _, found, wide = _split_task("cuts", "below_depth", 2048)
    assert not found and not wide and q == pout - 512 and is_cut("below_depth")[pout - 1025] and not is_cut("below_depth")[pout - 1024:pout].any()
    # pout itself and nothing else in range: none
    q, pout, _, found, _ = _split_task("cuts", "only_pout", 2048)
    assert not found and q == pout - 512 and is_cut("only_pout")[pout] and not is_cut("only_pout")[pout - 1024:pout].any()
    # pout - 1
    assert _split_task("cuts", "lanes", 256)[0] == 255
    # pout <= depth + 258: the scan starts at the block's first position and takes a cut point below pout - depth
    q, pout, _, found, _ = _split_task("cuts", "run_row_64", 1280)
    assert found and q == 99 and q < 258 and q < pout - 1024 and pout <= 1024 + 258 and cc.scan_start(pout, 1024, 512) == 0
    q, pout, _, found, _ = _split_task("cuts", "q1", 256)
    assert found and q == 1


@pytest.mark.parametrize("depth", [1, 63, 64, 65, 1024])
def test_search_depths(depth):
    """Block "depths": the last cut point before task 512 lies 1 before it, before 768, 1024, 1280, 1536: 2, 63, 64, 65,
    and the one before that at least 89 back."""
    case = "cuts" if depth == 1024 else f"cuts_depth_{depth}"
    assert cc.knobs(case)["cuts"] == depth and cc.CASES[case][0] == "cuts"
    for pout, back in ((512, 1), (768, 2), (1024, 63), (1280, 64), (1536, 65)):
        q, _, _, found, wide = _split_task(case, "depths", pout)
        assert found == (back <= depth) and not wide and q == (pout - back if found else pout - 512), (pout, q)
    if depth < 1024:
        is_cut = cc.cut_points(_block("cuts", "depths")[2]["kend"])
        assert all(not is_cut[pout - 88:pout - back].any() for pout, back in ((1024, 63), (1280, 64), (1536, 65)))


def test_no_search():
    """ZOPFLI_AMD_SEG_CUTS=0: the plain split.  A block below two task lengths and an empty block between others have
    one task; the first task behind the head of a later block finds its cut point."""
    ref, d = cc.reference("cuts_off"), cc.data("cuts")
    assert ref["found"] == 0 and ref["merged"] == 0
    want = [[b, q, pout, pend] for b, B in enumerate(d.sizes) for q, pout, pend in cc.split(B, 256, 256, 512)]
    assert ref["tasks"].tolist() == want and len(want) > cc.reference("cuts")["merged"] + len(cc.reference("cuts")["tasks"]) - 1
    assert any(q == pout - 512 > 0 for _, q, pout, _ in want)
    main = cc.reference("cuts")
    for name, B in (("one_task", 400), ("empty", 0)):
        b = d.names[name]
        assert 0 < b < len(d.blocks) - 1 and d.sizes[b] == B and main["split"][b] == [[0, 0, B + 1, False, False]]
    assert sum(bool(rows[1][3]) for b, rows in enumerate(main["split"]) if b >= 1 and len(rows) > 1) >= 10


# ------------------------------------------------------------------------------------------------ wide and merge
def _material(name, lo, hi, mutant=None):
    return cc.long_run_material(_block("cuts", name)[2], mutant)[lo:hi]


def test_wide_by_shortcut_positions_and_chains_of_merges():
    for name, wide_tasks, pend in (("wide3", (1536, 1792, 2048), 2304), ("wide2", (1536, 1792), 2048)):
        lay = _block("cuts", name)[2]
        for pout in wide_tasks:
            q, _, _, found, wide = _split_task("cuts", name, pout)
            assert not found and wide and lay["shortcut"][pout - 512:pout].any()
        assert [r[4] for r in cc.reference("cuts")["split"][cc.data("cuts").names[name]]].count(True) == len(wide_tasks)
        assert _kept_task("cuts", name, 1280)[2] == pend and all(r[1] not in wide_tasks for r in _kept("cuts", name))


def test_wide_by_run_rows_at_the_threshold():
    for name, longest, merged in (("run_row_64", 64, True), ("run_row_63", 63, False)):
        lay = _block("cuts", name)[2]
        q, pout, _, found, wide = _split_task("cuts", name, 1536)
        rows = lay["kend"][pout - 512:pout][lay["run_row"][pout - 512:pout] != 0]
        assert not lay["shortcut"].any() and int(rows.max()) == longest
        assert not found and wide == merged and q == pout - 512
        assert _kept_task("cuts", name, 1280)[2] == (1792 if merged else 1536)
        assert any(r[1] == 1536 for r in _kept("cuts", name)) != merged


def test_material_outside_the_warm_up_stretch_or_before_a_cut_point():
    q, pout, _, found, wide = _split_task("cuts", "far_material", 2048)
    assert not found and not wide and q == 1536
    assert _material("far_material", pout - 1024, pout - 512).any() and not _material("far_material", pout - 512, pout).any()
    q, pout, _, found, wide = _split_task("cuts", "cut_behind", 2048)
    assert found and not wide and q == 1948 and _material("cut_behind", pout - 512, q).any()
    assert _kept_task("cuts", "cut_behind", 2048)[0] == 1948


def test_merges_at_block_ends():
    """The last task of "last_wide" is wide: its predecessor ends at B + 1.  The block behind it begins with two wide
    tasks: ITS head takes them."""
    d = cc.data("cuts")
    assert d.names["head_wide"] == d.names["last_wide"] + 1
    assert _split_task("cuts", "last_wide", 1536)[2:] == [2001, False, True]
    assert _kept("cuts", "last_wide")[-1][:3] == [201, 1280, 2001]
    assert [r[4] for r in cc.reference("cuts")["split"][d.names["head_wide"]]] == [False, True, True, False]
    assert [r[:3] for r in _kept("cuts", "head_wide")] == [[0, 0, 768], [767, 768, 1101]]


def test_warm_up_longer_than_the_search():
    """ZOPFLI_AMD_SEG_WARM=1024 with ZOPFLI_AMD_SEG_CUTS=64, task 2048 of "far_material": no cut point within 64, run
    rows only in [pout - 1024, pout - 322), which a scan from pout - 64 - 258 on never meets.  By the documented rule
    the task is wide and merged."""
    assert cc.knobs("long_warm") == dict(seg_l=256, cuts=64, warm=1024, stretch=4)
    q, pout, _, found, wide = _split_task("long_warm", "far_material", 2048)
    assert not found and wide
    assert _material("far_material", pout - 1024, pout - 322).any() and not _material("far_material", pout - 322, pout).any()
    assert all(r[1] != 2048 for r in _kept("long_warm", "far_material"))
    assert cc.scan_start(pout, 64, 1024) == pout - 1024 < pout - 64 - 258


# ------------------------------------------------------------------------------------------------ k_taskkind
KINDS = "kinds_stretch_4"


def _classes(name, q, pend):
    _, B, lay = _block("kinds", name)
    return (lay["winflag"][q >> 5:(min(pend, B) + 31) >> 5] & 0xff).tolist()


def test_kind_thresholds():
    assert cc.knobs(KINDS)["seg_l"] == 512
    q, pout, pend, kind, g, n = _kept("kinds_stretch_4", "g4_of_16")[0]
    assert (kind, g, n) == (1, 4, 16) and sorted(set(_classes("g4_of_16", q, pend))) == [1, 2, 3]     # every generic window is of class 3
    assert _kept_task(KINDS, "g4_of_17", 512)[3:] == [0, 4, 17]
    q, pout, pend, kind, g, n = _kept(KINDS, "g3_of_12")[0]
    assert (kind, g, n) == (0, 3, 12) and 4 * g >= n >= 8
    q, pout, pend, kind, g, n = _kept(KINDS, "class2")[0]
    cls = _classes("class2", q, pend)
    assert (kind, g, n) == (0, 0, 16) and cls.count(2) >= 4 and set(cls) <= {1, 2}


def test_kind_windows_at_both_ends():
    # q is no multiple of 32 and the window that holds it is one of five generic ones in 20
    q, pout, pend, kind, g, n = _kept_task(KINDS, "q_window", 1024)
    assert q % 32 and (kind, g, n) == (1, 5, 20) and _classes("q_window", q, pend)[0] == 3
    # a block's only and last task: the partial last window is of class 0 and counts, the record behind it does not
    for name, want in (("g4_partial", (1, 4, 16)), ("g3_of_12", (0, 3, 12))):
        _, B, lay = _block("kinds", name)
        (q, pout, pend, kind, g, n), = _kept(KINDS, name)
        assert B % 32 and pend == B + 1 and (kind, g, n) == want and _classes(name, q, pend)[-1] == 0
        assert len(lay["winflag"]) == n + 1 and int(lay["winflag"][n]) & 0xff == 0


def test_kind_of_long_merged_tasks():
    q, pout, pend, kind, g, n = _kept_task(KINDS, "stride_64", 1024)
    assert 64 < n <= 128 and kind == 0 and pend == 3601
    q, pout, pend, kind, g, n = _kept_task(KINDS, "stride_128", 1024)
    assert n > 128 and kind == 1 and pend == 6401 and q % 32
    assert cc.reference(KINDS)["merged"] == 4 + 9


def test_no_text_task():
    ref = cc.reference("all_runs")
    assert ref["kind"].tolist() == [1] * 5 and ref["n_wg"] == 0 and ref["n_wg_runs"] == 4 and ref["merged"] == 1
    assert any(int(q) % 32 for _, q, _, _ in ref["tasks"])


# ------------------------------------------------------------------------------------------------ the lists
@pytest.mark.parametrize("stretch", [1, 3, 4, 5])
def test_lists_interleave(stretch):
    """Block "interleave": eleven tasks, run and text in turn, the head a run task: six run tasks and five text tasks
    in stretches of 1, 3, 4 and 5 leave remainders of every size; the batch also holds blocks of one task, an empty one
    and heads of both kinds."""
    case = f"kinds_stretch_{stretch}"
    ref, d = cc.reference(case), cc.data("kinds")
    assert cc.knobs(case)["stretch"] == stretch
    assert [r[3] for r in _kept(case, "interleave")] == [1, 0] * 5 + [1]
    a0 = int(ref["task_off"][d.names["interleave"]])
    desc, n_wg = ref["wg_desc"].astype(int), ref["n_wg"]
    sizes = {0: [], 1: []}
    for i, (first, n) in enumerate(desc):
        held = ref["wg_tasks"][first:first + n].astype(int)
        if a0 <= held[0] < a0 + 11:
            sizes[int(i >= n_wg)].append(int(n))
    assert sorted(sizes[0]) == sorted([stretch] * (5 // stretch) + [5 % stretch] * (5 % stretch > 0))
    assert sorted(sizes[1]) == sorted([stretch] * (6 // stretch) + [6 % stretch] * (6 % stretch > 0))
    # among the workgroups of a kind those that hold a head come first: every block's head is held by one of them
    heads = set(map(int, ref["task_off"][:-1]))
    for lo, hi in ((0, n_wg), (n_wg, len(desc))):
        holds = [int(ref["wg_tasks"][first]) in heads for first, _ in desc[lo:hi]]
        assert holds == sorted(holds, reverse=True) and any(holds) and not all(holds)
    one_task = [b for b in range(len(d.sizes)) if ref["task_off"][b + 1] - ref["task_off"][b] == 1]
    assert any(d.sizes[b] == 0 for b in one_task) and any(d.sizes[b] > 0 for b in one_task)


# ------------------------------------------------------------------------------------------------ wrong variants
MUTANT_CASE = {
    "admit_pout": "cuts", "strict_lower": "cuts", "drop_exact_depth": "cuts", "wide_from_63": "cuts",
    "wide_ignores_run_rows": "cuts", "warm_unseen": "long_warm", "merge_keeps_pend": "cuts", "class3_is_text": KINDS,
    "class2_is_generic": KINDS, "no_g_floor": KINDS, "kind_w0_rounds_up": KINDS, "kind_drops_partial": KINDS,
    "kind_counts_past_end": KINDS, "kind_first_64": KINDS, "kind_first_128": KINDS, "heads_not_first": KINDS,
    "stretch_spans_kinds": KINDS,
}
# the block and task at which the variant must differ from the reference (kinds: whose kind flips)
MUTANT_TASK = {
    "admit_pout": ("only_pout", 2048), "strict_lower": ("run_row_64", 1280), "drop_exact_depth": ("exact_depth", 2048),
    "class3_is_text": ("g4_of_16", 0), "class2_is_generic": ("class2", 0), "no_g_floor": ("g3_of_12", 0),
    "kind_w0_rounds_up": ("q_window", 1024), "kind_drops_partial": ("g4_partial", 0), "kind_counts_past_end": ("g3_of_12", 0),
    "kind_first_64": ("stride_64", 1024), "kind_first_128": ("stride_128", 1024),
}


def test_every_wrong_variant_is_listed():
    assert set(MUTANT_CASE) == set(cc.MUTANTS)


@pytest.mark.parametrize("mutant", cc.MUTANTS)
def test_a_case_tells_the_wrong_variant(mutant):
    case = MUTANT_CASE[mutant]
    right, wrong = cc.reference(case), cc.reference(case, mutant)
    assert cc.first_difference(wrong, right) is not None
    if mutant in MUTANT_TASK:
        name, pout = MUTANT_TASK[mutant]
        b = cc.data(cc.CASES[case][0]).names[name]
        if case == KINDS:
            kind_of = lambda ref: [int(ref["kind"][i]) for i in range(len(ref["tasks"]))      # noqa: E731
                                   if (int(ref["tasks"][i][0]), int(ref["tasks"][i][2])) == (b, pout)]
            assert len(kind_of(right)) == 1 and kind_of(right) != kind_of(wrong)
        else:
            one = lambda ref: [r[:4] for r in ref["split"][b] if r[1] == pout]      # noqa: E731
            assert len(one(right)) == 1 and one(right) != one(wrong)
    if mutant == "warm_unseen":
        assert wrong["merged"] < right["merged"]


# ------------------------------------------------------------------------------------------------ the quality pin
def test_text_tasks_start_at_cut_points():
    """Class T under the default search depth and warm-up: all tasks but the heads, or all but one of them, start at a
    cut point.  test_gpu_chain_tasks.py holds the device to the same count."""
    ref = cc.reference("text")
    assert cc.CASES["text"][1]["cuts"] is None and cc.CASES["text"][1]["warm"] is None
    others = sum(len(rows) - 1 for rows in ref["split"])
    assert others >= 80 and ref["found"] >= others - 1 and ref["merged"] == 0
