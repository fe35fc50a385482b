"""How the table build cuts the DP chain into tasks — the split (BuildChainTasks), the tasks' starts at cut points and
the "wide" mark (k_cutpoints), the merge of wide tasks into their predecessors, the tasks' kinds (k_taskkind) and the
workgroup lists (BuildWorkgroupLists); Tables.chain_tasks reads it back — as a plain reference in numpy, and inputs
glued so that the cut points land where a case needs them.

reference_tasks is written from DESIGN.md section 4 and the comments of zmx_dp_build.h and drv_build.h: a cut point is
taken from the TRUE prefix maximum over the whole block, not from a windowed one.  Per block it takes kend, shortcut,
run_row and winflag from dp_row_cases.reference_layout, to which test_gpu_dp_rows.py already holds the device.
windowed_last_cut restates the kernel's scan in 64-position chunks, with a switch that drops the carry between chunks:
test_cpu_chain_task_cases.py uses it to show where a chunk edge or the carry decides, and that with the carry it
equals the definition.  `mutant` names a deliberately wrong variant of the reference; the CPU test shows for every one
that some case tells it from the right one, so a device that made the same mistake would fail on that case.

No device is involved here.  Everything is computed once per process (functools.lru_cache) and must be left unchanged
by its users."""
import functools

import numpy as np

import dp_row_cases as dc
from zopfli_amd import generate

MAX_MATCH = 258
WIDE_RUN = 64            # a run row of this many edges or more is long-run material (k_cutpoints, k_mkdesc)
DEFAULT_CUTS, DEFAULT_WARM = 1024, 512

MUTANTS = ("admit_pout", "strict_lower", "drop_exact_depth", "wide_from_63", "wide_ignores_run_rows", "warm_unseen",
           "merge_keeps_pend", "class3_is_text", "class2_is_generic", "no_g_floor", "kind_w0_rounds_up",
           "kind_drops_partial", "kind_counts_past_end", "kind_first_64", "kind_first_128", "heads_not_first",
           "stretch_spans_kinds")


# ------------------------------------------------------------------------------------------------ the reference
def knob_warm(v):
    """ZOPFLI_AMD_SEG_WARM as zmx_knobs.h states it: 64 .. 2^20, rounded up to 64."""
    return (min(max(int(v), 64), 1 << 20) + 63) & ~63


def split(B, L, head, warm):
    """BuildChainTasks: [q, pout, pend] of the block's tasks before any cut point is looked for."""
    n = 1 if L == 0 or B < head + L else 1 + (B - head) // L
    out = []
    for s in range(n):
        pout = 0 if s == 0 else head + (s - 1) * L
        out.append([pout - min(warm, pout), pout, B + 1 if s + 1 == n else head + s * L])
    return out


def cut_points(kend):
    """is_cut[q] for q = 0 .. B: no DP edge crosses q — p + kend(p) <= q for every p < q.  (q = 0 is no cut point:
    nothing starts before it.)"""
    kend = np.asarray(kend, dtype=np.int64)
    B = len(kend)
    out = np.zeros(B + 1, dtype=bool)
    if B:
        reach = np.maximum.accumulate(np.arange(B, dtype=np.int64) + kend)     # reach[q - 1]: the furthest cell an edge from below q gets to
        out[1:] = reach <= np.arange(1, B + 1)
    return out


def search_floor(pout, depth):
    """The smallest q a task may take: pout - depth, and 1 where pout <= depth + 258 (the scan then covers the block
    from its first position on and any older cut point is as exact)."""
    return 1 if pout <= depth + MAX_MATCH else pout - depth


def last_cut(is_cut, pout, depth, mutant=None):
    """The last cut point q with max(1, floor) <= q < pout, or None."""
    if depth == 0 or pout == 0:
        return None
    lo = max(pout - depth, 1) if mutant == "strict_lower" else search_floor(pout, depth)
    if mutant == "drop_exact_depth" and lo > 1:
        lo += 1
    hi = pout + 1 if mutant == "admit_pout" else pout
    at = np.flatnonzero(is_cut[lo:hi])
    return int(lo + at[-1]) if len(at) else None


def long_run_material(lay, mutant=None):
    kend = lay["kend"].astype(np.int64)
    rows = (lay["run_row"] != 0) & (kend >= (63 if mutant == "wide_from_63" else WIDE_RUN))
    if mutant == "wide_ignores_run_rows":
        rows[:] = False
    return (lay["shortcut"] != 0) | rows


def task_kind(q, pend, B, winflag, mutant=None):
    """-> (kind, g, windows) of one task."""
    w0 = (q + 31) >> 5 if mutant == "kind_w0_rounds_up" else q >> 5
    end = min(pend, B)
    w1 = end >> 5 if mutant == "kind_drops_partial" else (end + 31) >> 5
    if mutant == "kind_counts_past_end" and pend > B:
        w1 += 1
    if mutant == "kind_first_64":
        w1 = min(w1, w0 + 64)
    if mutant == "kind_first_128":
        w1 = min(w1, w0 + 128)
    cls = np.asarray(winflag[w0:w1]).astype(np.int64) & 0xff
    generic = (cls == 0) | (cls == (2 if mutant == "class2_is_generic" else 3))
    if mutant == "class3_is_text":
        generic = cls == 0
    g, n = int(generic.sum()), max(w1 - w0, 0)
    return (1 if 4 * g >= n and (g >= 4 or mutant == "no_g_floor") else 0), g, n


def reference_tasks(lays, sizes, knobs, mutant=None):
    """What Tables.chain_tasks() must return for blocks of `sizes` positions whose reference layouts are `lays`, under
    knobs = dict(seg_l, cuts, warm, stretch) (ZOPFLI_AMD_SEG_HEAD = 0 and fewer than 48 blocks: the head is as long as
    a task), as a dict of the same names; and with it "split" (per block the tasks before the merge: [q, pout, pend,
    found, wide]), "found" (tasks of the split that start at a cut point) and "g" / "windows" per task."""
    L, depth, warm, S = knobs["seg_l"], knobs["cuts"], knob_warm(knobs["warm"]), knobs["stretch"]
    head = max(0, L)
    tasks, task_off, per_block, merged, found = [], [0], [], 0, 0
    for b, (B, lay) in enumerate(zip(sizes, lays)):
        is_cut = cut_points(lay["kend"])
        material = long_run_material(lay, mutant)
        rows = []
        for q, pout, pend in split(B, L, head, warm):
            cut = last_cut(is_cut, pout, depth, mutant)
            wide = False
            if depth and pout and cut is None:
                lo = pout - min(warm, pout)
                if mutant == "warm_unseen":
                    lo = max(lo, pout - depth - MAX_MATCH)
                wide = bool(material[lo:pout].any())
            rows.append([q if cut is None else cut, pout, pend, cut is not None, wide])
            found += cut is not None
        per_block.append(rows)
        kept = []
        for i, (q, pout, pend, _, wide) in enumerate(rows):
            if wide and i > 0:                  # (a head is never wide: it has nothing to search)
                if mutant != "merge_keeps_pend":
                    kept[-1][3] = pend
                merged += 1
            else:
                kept.append([b, q, pout, pend])
        tasks += kept
        task_off.append(len(tasks))
    kind, gs, ns = [], [], []
    for b, q, pout, pend in tasks:
        k, g, n = task_kind(q, pend, sizes[b], lays[b]["winflag"], mutant)
        kind.append(k)
        gs.append(g)
        ns.append(n)
    lists = [[], []]
    desc = [[[], []], [[], []]]                 # [kind][0: holds the block's head, 1: the others]
    for b in range(len(sizes)):
        a0, a1 = task_off[b], task_off[b + 1]
        for kd in (0, 1):
            if mutant == "stretch_spans_kinds" and kd == 1:
                continue
            l0 = len(lists[kd])
            lists[kd] += [k for k in range(a0, a1) if kind[k] == kd or mutant == "stretch_spans_kinds"]
            l1 = len(lists[kd])
            for i in range(l0, l1, S):
                holds_head = i == l0 and lists[kd][l0] == a0 and mutant != "heads_not_first"
                desc[kd][0 if holds_head else 1].append((i, min(S, l1 - i)))
    shift = len(lists[0])
    wg = desc[0][0] + desc[0][1] + [(i + shift, n) for i, n in desc[1][0] + desc[1][1]]
    u32 = lambda x, shape: np.asarray(x, dtype=np.uint32).reshape(shape)    # noqa: E731
    return dict(tasks=u32(tasks, (-1, 4)), task_off=u32(task_off, -1), merged=merged, kind=u32(kind, -1),
                wg_tasks=u32(lists[0] + lists[1], -1), wg_desc=u32(wg, (-1, 2)), n_wg=len(desc[0][0]) + len(desc[0][1]),
                n_wg_runs=len(desc[1][0]) + len(desc[1][1]), split=per_block, found=found, g=gs, windows=ns)


def first_difference(got, want):
    """None, or what differs first between Tables.chain_tasks() and reference_tasks(...)."""
    for name in ("merged", "n_wg", "n_wg_runs"):
        if int(got[name]) != int(want[name]):
            return f"{name} {int(got[name])}, reference {int(want[name])}"
    for name in ("task_off", "tasks", "kind", "wg_tasks", "wg_desc"):
        g, w = np.asarray(got[name]), np.asarray(want[name])
        if g.shape != w.shape:
            return f"{name} has shape {g.shape}, reference {w.shape}"
        bad = np.argwhere(g != w)
        if len(bad):
            i = tuple(map(int, bad[0]))
            row = f" (row {g[i[0]].tolist()}, reference {w[i[0]].tolist()})" if g.ndim == 2 else ""
            return f"{name}{list(i)}: {int(g[i])}, reference {int(w[i])}{row} ({len(bad)} differ)"
    return None


def scan_start(pout, depth, warm):
    """Where k_cutpoints' scan of a task begins: 258 positions before the lowest q it may take (0 where that floor is
    1), or at the start of the warm-up stretch where that lies further back."""
    lo = pout - depth - MAX_MATCH if pout > depth + MAX_MATCH else 0
    return min(lo, pout - min(warm, pout))


def windowed_last_cut(kend, pout, depth, warm, carry=True):
    """The scan as zmx_dp_build.h describes it: 64 positions at a time from scan_start on, a prefix maximum of p + kend
    inside a chunk, the maximum so far carried from chunk to chunk (carry=False: dropped), q = p + 1 taken when the
    maximum is at most q, q < pout, and q is at least 258 beyond the unwindowed lower end (1 where that is 0)."""
    kend = np.asarray(kend, dtype=np.int64)
    lo = pout - depth - MAX_MATCH if pout > depth + MAX_MATCH else 0
    q_min = 1 if lo == 0 else lo + MAX_MATCH
    best, over = None, 0
    for p0 in range(scan_start(pout, depth, warm), pout, 64):
        p = np.arange(p0, min(p0 + 64, pout), dtype=np.int64)
        incl = np.maximum(np.maximum.accumulate(p + kend[p]), over if carry else 0)
        ok = np.flatnonzero((p + 1 < pout) & (p + 1 >= q_min) & (incl <= p + 1))
        if len(ok):
            best = int(p[ok[-1]] + 1)
        over = int(incl[-1])
    return best


# ------------------------------------------------------------------------------------------------ gluing
class Block:
    """One block glued from random bytes (almost every position a cut point), copies of spans that lie in a pool in
    front of the block (no cut point strictly inside, one at the end) and runs of one byte.  The pool is no part of
    the block; every copy gets a fresh span of it, fenced so that the copy begins and ends exactly where asked."""

    def __init__(self, rng, lead=b""):
        self.rng, self.pool, self.body, self.lead = rng, bytearray(), bytearray(), bytes(lead)   # lead: the bytes just before the block
        self._cont = None        # index in pool of the byte that continues the last copy: the next byte must differ
        self._avoid = None       # the byte of the run that has just ended: the next byte must differ
        self._glue = None        # the byte of a run whose end the next copy takes in

    def _fresh(self, n):
        return bytearray(self.rng.integers(0, 256, n, dtype=np.uint8).tobytes())

    def _first(self, byte):
        """The next byte of the body is `byte`: the copy before it must not go on through it."""
        if self._cont is not None and self.pool[self._cont] == byte:
            self.pool[self._cont] ^= 0x55
        self._cont = None

    def rand(self, to):
        b = self._fresh(to - len(self.body))
        if len(b):
            if self._avoid is not None and b[0] == self._avoid:
                b[0] ^= 0x55
            self._first(b[0])
            self._avoid = None
            self.body += b
        return self

    def run(self, to, c, glued=False, goes_on=False):
        """Equal bytes up to `to`.  goes_on: the bytes before are c already (the tail of a copy, the lead);
        glued: the next copy takes the run's end in, so that no cut point follows the run."""
        assert goes_on == (bool(self.body[-1:] == bytes([c])) if self.body else self.lead[-1:] == bytes([c])), len(self.body)
        self._first(c)
        self.body += bytes([c]) * (to - len(self.body))
        self._avoid, self._glue = (None, c) if glued else (c, None)
        return self

    def copy(self, to, end_with=b"", overlap=0):
        """A copy up to `to` of a fresh span of the pool.  end_with: its last bytes (the first bytes of a run that
        follows, so that no cut point lies at the run's start); overlap: it begins that many bytes before the cursor,
        with the bytes that stand there, so that no cut point lies where the copy before it ends."""
        m = to - len(self.body)
        assert m >= 3 and (overlap == 0 or self._glue is None)
        front = bytes([self._glue] * 2) if self._glue is not None else bytes(self.body[len(self.body) - overlap:])
        k = len(front)
        T = bytearray(front) + self._fresh(m + 1)
        if end_with:
            T[k + m - len(end_with):k + m] = end_with
        differ = self._glue if self._glue is not None else self._avoid
        if differ is not None and T[k] == differ:
            T[k] ^= 0x55
        if T[k + m] == T[k + m - 1]:          # (the byte behind the copy in the pool must not go on with a run)
            T[k + m] ^= 0x55
        before = self.body[len(self.body) - overlap - 1] if len(self.body) > overlap else 0x5a
        guard = (front[0] if self._glue is not None else before) ^ 0xff
        self._first(T[k])
        self.pool += bytes([guard]) + T
        self._cont = len(self.pool) - 1
        self.body += T[k:k + m]
        self._avoid = self._glue = None
        return self

    def chain(self, to, unit=40):
        """Copies of `unit` bytes, each begun on the last byte of the one before: no cut point up to `to`."""
        while len(self.body) < to:
            step = min(unit, to - len(self.body))
            if to - len(self.body) - step in (1, 2):
                step += to - len(self.body) - step
            self.copy(len(self.body) + step, overlap=0 if self._glue is not None else 1)
        return self

    def short_run(self, at, n, c):
        """n bytes c from `at` on with no cut point before, inside or behind: a copy ends with the first three, the
        next copy takes the end in."""
        self.copy(at + 3, end_with=bytes([c]) * 3, overlap=0 if self._glue is not None else 1)
        return self.run(at + n, c, glued=True, goes_on=True)


class Batch:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.data, self.blocks, self.names = bytearray(), [], {}

    def add(self, name, block):
        assert name not in self.names
        self.names[name] = len(self.blocks)
        self.data += block.pool + block.lead
        self.blocks.append((len(self.data), len(self.data) + len(block.body)))
        self.data += block.body

    def new(self, lead=b""):
        return Block(self.rng, lead)


class Data:
    def __init__(self, data, blocks, names):
        self.data, self.blocks, self.names = bytes(data), list(blocks), dict(names)
        self.sizes = [e - s for s, e in self.blocks]
        assert len(self.data) <= 65536


def _cuts_data():
    """SEG_L = 256, so the tasks own [256 k, 256 k + 256).  What every block is for is asserted in
    test_cpu_chain_task_cases.py, under the knobs named there."""
    t = Batch(21)
    # the chosen cut point on lane 0 (task 2048: q = 1087) and on lane 63 (task 3072: q = 2430) of a chunk; behind random
    # bytes q = pout - 1, which the last, partial chunk of a scan holds
    t.add("lanes", t.new().rand(1087).copy(2090).rand(2430).copy(3100).rand(3400))
    t.add("exact_depth", t.new().rand(500).copy(1024).copy(2100).rand(2400))           # task 2048: its only cut point is pout - 1024
    t.add("below_depth", t.new().rand(500).copy(1023).copy(2100).rand(2400))           # ... is pout - 1025: none
    t.add("only_pout", t.new().rand(500).copy(1000).copy(2048).copy(2100).rand(2400))  # ... is pout itself: none
    # a copy of 200 bytes from 1720 on ends two positions into a chunk of task 2048's scan, the next copy begins on its
    # last byte: without the carry 1919 looks like a cut point
    t.add("carry", t.new().rand(1720).copy(1920).copy(2100, overlap=1).copy(2330).rand(2700))
    t.add("q1", t.new().rand(1).copy(300).rand(600))                                   # task 256: q = 1
    # cut points 1, 2, 63, 64 and 65 before tasks 512 .. 1536 and nothing else within 88: SEG_CUTS = 1, 63, 64, 65
    t.add("depths", t.new().rand(300).copy(400).copy(511).copy(600).copy(766).copy(800).copy(961).copy(1100).copy(1216)
          .copy(1400).copy(1471).copy(1600).rand(1900))
    t.add("one_task", t.new().rand(400))
    t.add("empty", t.new())
    # long runs: tasks 1536, 1792, 2048 (two of them in the second block) find no cut point and shortcut positions behind them
    t.add("wide3", t.new().rand(200).run(2200, 0x11).rand(2800))
    t.add("wide2", t.new().rand(200).run(1950, 0x22).rand(2600))
    # 65 equal bytes (the longest run row: 64 edges) and 64 (63 edges) with no cut point before, inside or behind
    b = t.new().rand(100).chain(1297, unit=200)
    t.add("run_row_64", b.short_run(1297, 65, 0x33).chain(1700, unit=200).rand(2100))
    b = t.new().rand(100).chain(1297, unit=200)
    t.add("run_row_63", b.short_run(1297, 64, 0x44).chain(1700, unit=200).rand(2100))
    # a run of 303 bytes in [1145, 1448): inside task 2048's search range, before its warm-up stretch of 512 — and inside
    # a warm-up stretch of 1024 that a search depth of 64 does not reach
    b = t.new().rand(500).chain(1145, unit=200)
    t.add("far_material", b.short_run(1145, 303, 0x55).chain(2100, unit=200).rand(2400))
    # a run in task 2048's warm-up stretch that ends at 1948 in a cut point
    b = t.new().rand(300).chain(1497, unit=200).copy(1500, end_with=b"\x66" * 3, overlap=1)
    t.add("cut_behind", b.run(1948, 0x66, goes_on=True).copy(2100).rand(2400))
    # the block ends inside a run: its last task (1536) is wide; then a block that begins inside one: tasks 256 and 512 are
    t.add("last_wide", t.new().rand(200).run(2000, 0x77))
    t.add("head_wide", t.new(lead=b"\x88" * 8).run(700, 0x88, goes_on=True).rand(1100))
    return Data(t.data, t.blocks, t.names)


def _class3(block, at, windows):
    """A copy from `at` (a multiple of 32) on that makes exactly `windows` windows of class 3: its rows reach 128 and
    more positions ahead in those and fewer behind them."""
    assert at % 32 == 0
    return block.copy(at + 32 * windows + 98)


def _kinds_data():
    """SEG_L = 512: a head owns 16 windows."""
    t = Batch(22)
    t.add("g4_of_16", _class3(t.new().rand(64), 64, 4).rand(1100))                     # the head: 4 windows of class 3 in 16
    t.add("g4_of_17", _class3(t.new().rand(608), 608, 4).rand(1600))                   # task 512 from q = 511: 4 in 17
    t.add("g3_of_12", _class3(t.new().rand(64), 64, 2).rand(380))                      # one task: 2 of class 3 and the partial window, of 12
    t.add("g4_partial", _class3(t.new().rand(64), 64, 3).rand(500))                    # one task: 3 of class 3 and the partial window, of 16
    b = t.new().rand(32)
    for at in range(132, 1033, 100):
        b.copy(at)
    t.add("class2", b.rand(1100))                                                      # the head: windows of class 2, none generic
    # the last task, 1024, starts at q = 1000 inside a window of class 3: with the partial last window 5 of 20
    t.add("q_window", _class3(t.new().rand(800).copy(1000), 1000 - 8, 4).rand(1630))
    # task 1024 starts at 101 in a run and, merged with four wide tasks, ends with the block: 110 windows, the generic
    # ones among the first 64
    b = t.new().rand(100).run(700, 0x12, glued=True)
    for at in (1100, 1600, 2100, 2600):
        b.chain(at).short_run(at, 65, 0x13)
    t.add("stride_64", b.chain(3200).rand(3600))
    # task 1024 starts at 100 and, merged with ten wide tasks, ends with the block inside a long run: 197 windows, the
    # generic ones beyond the first 128
    b = t.new().rand(100)
    for at in range(1100, 4101, 500):
        b.chain(at).short_run(at, 65, 0x14)
    b.chain(4297).copy(4300, end_with=b"\x15" * 3, overlap=1)
    t.add("stride_128", b.run(6400, 0x15, goes_on=True))
    t.add("empty", t.new())
    # eleven tasks: run, text, run, .. — the head is a run task and the lists of both kinds interleave
    b = t.new()
    for i in range(0, 11, 2):
        b.rand(512 * i + 6).run(512 * i + 470, 0x20 + i).rand(min(512 * (i + 2), 5732))
    t.add("interleave", b)
    return Data(t.data, t.blocks, t.names)


def _all_runs_data():
    """Every window of every block is generic: there is no text task."""
    t = Batch(23)
    t.add("whole_1200", t.new(lead=b"\x31" * 8).run(1200, 0x31, goes_on=True))
    t.add("whole_300", t.new(lead=b"\x32" * 8).run(300, 0x32, goes_on=True))
    t.add("from_40", t.new().rand(40).run(1500, 0x33))
    t.add("whole_700", t.new(lead=b"\x34" * 8).run(700, 0x34, goes_on=True))
    return Data(t.data, t.blocks, t.names)


TEXT_SEED = 5


def _text_data():
    """Class T, two blocks, the default search depth and warm-up."""
    return Data(generate("T", 24000, TEXT_SEED), [(0, 9000), (9000, 24000)], {})


_DATA = dict(cuts=_cuts_data, kinds=_kinds_data, all_runs=_all_runs_data, text=_text_data)


@functools.lru_cache(maxsize=None)
def data(name):
    return _DATA[name]()


@functools.lru_cache(maxsize=None)
def layouts(name):
    """reference_layout of every block (ZOPFLI_AMD_RUN_CODES unset: wide run rows take no codes)."""
    d = data(name)
    return [dc.reference_layout(d.data, s, e, True) for s, e in d.blocks]


# name -> (data, knobs); cuts / warm None: the library's defaults, the variable stays unset
CASES = {
    "cuts": ("cuts", dict(seg_l=256, cuts=1024, warm=512, stretch=4)),
    "cuts_depth_1": ("cuts", dict(seg_l=256, cuts=1, warm=512, stretch=4)),
    "cuts_depth_63": ("cuts", dict(seg_l=256, cuts=63, warm=512, stretch=4)),
    "cuts_depth_64": ("cuts", dict(seg_l=256, cuts=64, warm=512, stretch=4)),
    "cuts_depth_65": ("cuts", dict(seg_l=256, cuts=65, warm=512, stretch=4)),
    "cuts_off": ("cuts", dict(seg_l=256, cuts=0, warm=512, stretch=4)),
    "long_warm": ("cuts", dict(seg_l=256, cuts=64, warm=1024, stretch=4)),
    "kinds_stretch_1": ("kinds", dict(seg_l=512, cuts=1024, warm=512, stretch=1)),
    "kinds_stretch_3": ("kinds", dict(seg_l=512, cuts=1024, warm=512, stretch=3)),
    "kinds_stretch_4": ("kinds", dict(seg_l=512, cuts=1024, warm=512, stretch=4)),
    "kinds_stretch_5": ("kinds", dict(seg_l=512, cuts=1024, warm=512, stretch=5)),
    "all_runs": ("all_runs", dict(seg_l=512, cuts=1024, warm=512, stretch=4)),
    "text": ("text", dict(seg_l=256, cuts=None, warm=None, stretch=4)),
}


def knobs(case):
    k = dict(CASES[case][1])
    k["cuts"] = DEFAULT_CUTS if k["cuts"] is None else k["cuts"]
    k["warm"] = DEFAULT_WARM if k["warm"] is None else k["warm"]
    return k


def environment(case, base):
    """`base` with the case's knobs set, and unset where the case runs on the defaults."""
    env = dict(base)
    k = CASES[case][1]
    for var, v in (("SEG_L", k["seg_l"]), ("SEG_HEAD", 0), ("SEG_CUTS", k["cuts"]), ("SEG_WARM", k["warm"]),
                   ("SEG_STRETCH", k["stretch"])):
        env.pop("ZOPFLI_AMD_" + var, None)
        if v is not None:
            env["ZOPFLI_AMD_" + var] = str(v)
    return env


@functools.lru_cache(maxsize=None)
def reference(case, mutant=None):
    name = CASES[case][0]
    return reference_tasks(layouts(name), data(name).sizes, knobs(case), mutant)


# ------------------------------------------------------------------------------------------------ invariants
def is_cut_brute(kend, q):
    """The definition, position by position: q >= 1 and p + kend(p) <= q for every p < q."""
    return q >= 1 and all(p + int(kend[p]) <= q for p in range(q))


def invariants(ct, sizes, lays, knobs):
    """None, or the first rule that a task set-up (Tables.chain_tasks() or the reference's) breaks — stated without the
    reference: every task in exactly one descriptor, once; a descriptor holds at most `stretch` tasks of one block and
    one kind; the tasks of a block tile [0, B] and the last ends at B + 1; q <= pout; a q that is not the warm-up start
    is a cut point by the definition."""
    tasks, off = np.asarray(ct["tasks"]).astype(np.int64), np.asarray(ct["task_off"]).astype(np.int64)
    wg_tasks, desc = np.asarray(ct["wg_tasks"]).astype(np.int64), np.asarray(ct["wg_desc"]).astype(np.int64)
    nt, warm = len(tasks), knob_warm(knobs["warm"])
    if len(off) != len(sizes) + 1 or off[0] != 0 or off[-1] != nt or np.any(np.diff(off) < 1):
        return f"task_off {off.tolist()} for {nt} tasks"
    if len(desc) != ct["n_wg"] + ct["n_wg_runs"]:
        return f"{len(desc)} descriptors, n_wg {ct['n_wg']} + n_wg_runs {ct['n_wg_runs']}"
    seen = np.zeros(nt, dtype=np.int64)
    for i, (first, n) in enumerate(desc):
        if not (1 <= n <= knobs["stretch"] and 0 <= first and first + n <= len(wg_tasks)):
            return f"descriptor {i} = ({first}, {n})"
        held = wg_tasks[first:first + n]
        if held.min() < 0 or held.max() >= nt:
            return f"descriptor {i} holds {held.tolist()}"
        np.add.at(seen, held, 1)
        if len(set(tasks[held, 0])) != 1:
            return f"descriptor {i} spans blocks {sorted(set(tasks[held, 0]))}"
        if len(set(int(ct["kind"][k]) for k in held)) != 1 or int(ct["kind"][held[0]]) != (1 if i >= ct["n_wg"] else 0):
            return f"descriptor {i} mixes kinds or is listed with the other kind"
        if np.any(np.diff(held) <= 0):
            return f"descriptor {i} holds {held.tolist()}: not in order"
    if np.any(seen != 1):
        return f"task {int(np.flatnonzero(seen != 1)[0])} is in {int(seen[np.flatnonzero(seen != 1)[0]])} descriptors"
    for b, B in enumerate(sizes):
        rows = tasks[off[b]:off[b + 1]]
        if np.any(rows[:, 0] != b) or rows[0, 2] != 0 or rows[-1, 3] != B + 1 or np.any(rows[1:, 2] != rows[:-1, 3]):
            return f"the tasks of block {b} do not tile it: {rows.tolist()}"
        for _, q, pout, pend in rows:
            if q > pout or pend <= pout:
                return f"block {b}: task (q {q}, pout {pout}, pend {pend})"
            if q != pout - min(warm, pout) and not is_cut_brute(lays[b]["kend"], int(q)):
                return f"block {b}: q {q} of task {pout} is no cut point"
    return None
