"""The speculative pass of the chain by stretches (zmx_dp5_spec.h: k_dp5_spec, a task a wave, for stretches of up to four
tasks; k_dp5_stretch, where a workgroup sets up once and its waves pull the tasks of a stretch from a counter, for
longer ones, for the packed redo list and wherever ZOPFLI_AMD_SEG_PULL=1 asks for it), the packed redo list (zmx_dp4.h
k_dpscan) and the partial second check (k_dprecheck).  Every case goes through tests/chain_stretch_probe.py in a subprocess — the geometry is read once per
process — which runs three chained squeeze runs against the CPU oracle and reports zmx_last_seg_stats."""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

PROBE = os.path.join(os.path.dirname(__file__), "chain_stretch_probe.py")
SHORT = {"ZOPFLI_AMD_SEG_L": "256", "ZOPFLI_AMD_SEG_HEAD": "0"}


def probe(case, **env):
    r = subprocess.run([sys.executable, PROBE], env=dict(os.environ, STRETCH_PROBE_CASE=case, **env),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    st = json.loads(r.stdout.strip().splitlines()[-1])
    # ZOPFLI_AMD_PROF: every run reports the tasks k_dpscan listed for the redo pass and the entries it made of them
    lists = [(int(m.group(1)), int(m.group(2))) for m in re.finditer(r"redo list: (\d+) tasks in (\d+) entries", r.stderr)]
    st["redo_tasks"] = sum(a for a, _ in lists)
    st["redo_entries"] = sum(b for _, b in lists)
    st["redo_reports"] = len(lists)
    return st


def reruns(st):
    return st["rerun_state"] + st["rerun_level"] + st["rerun_tie"] + st["rerun_values"]


def consistent(st):
    """Every task but the heads (one per non-empty block and run, three runs) is accepted or run again, once."""
    return st["accepted"] + reruns(st) == st["tasks"] - 3 * st["blocks"]


# (stretch, ZOPFLI_AMD_SEG_PULL): up to four tasks a stretch k_dp5_spec runs the main pass unless the switch hands it to
# k_dp5_stretch, whose waves then find a stretch of 1 or 3 entries empty at their first pull
@pytest.mark.parametrize("stretch,pull", [("1", "0"), ("3", "0"), ("4", "0"), ("1", "1"), ("3", "1"), ("4", "1"),
                                          ("5", "0"), ("16", "0"), ("32", "0")])
def test_stretch_edges(stretch, pull):
    """Blocks of 1, 2, 4, 5, 6 and 17 tasks, an empty block and a 20-byte block in one batch, at stretches below, at and
    above the four waves of a workgroup and above every block's task count: with 1 and 3 entries, and in every
    stretch's remainder, waves find the stretch empty and leave at once while the others work."""
    st = probe("edges", ZOPFLI_AMD_SEG_STRETCH=stretch, ZOPFLI_AMD_SEG_PULL=pull, **SHORT)
    assert st["tasks"] == 3 * (1 + 2 + 4 + 5 + 6 + 1 + 17), st
    assert consistent(st), st


@pytest.mark.parametrize("int_path", ["1", "0"])
def test_binade_changes_inside_a_stretch(int_path):
    """One 64 KiB block of 256 tasks in stretches of 32: the level doubles several times inside a stretch, the integer
    table is that of the stretch's first speculative task and the tasks of the other binades walk in doubles."""
    st = probe("binade", ZOPFLI_AMD_SEG_STRETCH="32", ZOPFLI_AMD_INT_PATH=int_path, **SHORT)
    assert st["tasks"] == 3 * 256 and st["accepted"] > 0, st
    assert consistent(st), st


def test_mixed_kinds():
    """Text and long runs alternate in one block: text-kind and run-kind tasks interleave in the block's list, so the
    stretches of either kind are not contiguous in task index, and both variants of the kernel run."""
    st = probe("mixed", ZOPFLI_AMD_SEG_STRETCH="16")
    assert st["tasks"] > 3 * 20 and st["accepted"] > 0, st
    assert consistent(st), st


@pytest.mark.parametrize("redo", ["1", "2"])
def test_redo_packing_many(redo):
    """Every level guessed 1.9 times too high: many tasks per block are listed for the redo pass, packed four to an
    entry with a remainder; with two redo passes the second check empties the list's counter twice.  The profiling
    build reports what k_dpscan listed: two blocks and three runs make at most six entries that are not full."""
    st = probe("redo200k", ZOPFLI_AMD_SEG_SCALE="1.9", ZOPFLI_AMD_SEG_REDO=redo, ZOPFLI_AMD_PROF="1")
    assert st["rerun_level"] + st["rerun_values"] > 0 and st["accepted"] > 0, st
    assert consistent(st), st
    passes = 3 * 2 * int(redo)           # (runs x blocks x redo passes: each may leave one entry short of four tasks)
    assert st["redo_reports"] == 3 and st["redo_tasks"] > 4 * passes, st
    assert -(-st["redo_tasks"] // 4) <= st["redo_entries"] <= st["redo_tasks"] // 4 + passes, st


def test_redo_packing_few():
    """A 40 000-byte block with the levels as guessed: no listed task, or one or two, in as many entries as four to
    an entry make."""
    st = probe("redo40k", ZOPFLI_AMD_SEG_SCALE="1.0", ZOPFLI_AMD_PROF="1")
    assert st["accepted"] > 0, st
    assert consistent(st), st
    assert st["redo_reports"] == 3 and -(-st["redo_tasks"] // 4) <= st["redo_entries"] <= st["redo_tasks"], st


def test_partial_second_check():
    """After a redo pass only the checks of the listed tasks and their successors are computed again; a stale or missed
    chk[] entry would accept a task on the wrong shift or re-run it from the wrong state.  The outputs equal those of
    a process without redo passes, where everything undecided falls to the serial pass."""
    with_redo = probe("redo200k", ZOPFLI_AMD_SEG_SCALE="1.9", ZOPFLI_AMD_SEG_REDO="1")
    without = probe("redo200k", ZOPFLI_AMD_SEG_SCALE="1.9", ZOPFLI_AMD_SEG_REDO="0")
    assert with_redo["digest"] == without["digest"]
    assert without["rerun_level"] + without["rerun_values"] >= with_redo["rerun_level"] + with_redo["rerun_values"], (with_redo, without)
    assert consistent(with_redo) and consistent(without), (with_redo, without)


def test_redo_entries_of_one_task():
    """The redo pass of a table set with run tasks: every level guessed 1.9 times too high on the block of text and long
    runs, so k_dpscan lists tasks, a task an entry, and k_dp5_spec<.., true> runs them again from their own levels (no
    scale, through its redo entry path).  The outputs equal those of a process without redo passes."""
    st = probe("mixed", ZOPFLI_AMD_SEG_SCALE="1.9", ZOPFLI_AMD_PROF="1")
    print(st)
    assert consistent(st), st
    assert st["redo_reports"] == 3, st
    assert st["redo_tasks"] > 0, st
    assert st["redo_entries"] == st["redo_tasks"], st
    without = probe("mixed", ZOPFLI_AMD_SEG_SCALE="1.9", ZOPFLI_AMD_SEG_REDO="0")
    assert st["digest"] == without["digest"]


def test_stretch_edges_guarded():
    """The stretch-edges batch with red zones around every device allocation, checked after every launch."""
    st = probe("edges", ZOPFLI_AMD_SEG_STRETCH="16", ZOPFLI_AMD_GUARD="1", **SHORT)
    assert consistent(st), st
