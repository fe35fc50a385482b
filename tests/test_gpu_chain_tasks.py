"""The chain's task set-up as the table build leaves it — the split (BuildChainTasks), the starts at cut points and the
wide mark (k_cutpoints), the merge, the kinds (k_taskkind), the workgroup lists (BuildWorkgroupLists) — read back with
Tables.chain_tasks (zmx_chain_tasks_download) and held to the plain reference of chain_task_cases.py by integer
equality, on exactly the cases whose reach test_cpu_chain_task_cases.py asserts.  The parity tests cannot see any of
this: a wrong cut point, merge, kind or stretch only turns accepted tasks into serial re-runs.

The knobs are read once per process, so every case runs tests/chain_task_probe.py in a child process, one at a time,
which also takes the tables through three chained squeeze runs against the CPU oracle: the task geometries of these
cases (starts that are no multiple of 32, heads with tasks merged into them, tasks of thousands of positions, lists of
both kinds that interleave) are the ones the speculative kernels see least.

This comparison was seen to fail where it should: held against each of the seventeen deliberately wrong variants of
the reference (chain_task_cases.MUTANTS — q = pout admitted, class 3 counted as text, the unexamined part of a long
warm-up stretch, ...) the device's output of the case that test_cpu_chain_task_cases.py names for the variant differs,
e.g. "admit_pout" on "cuts" at tasks[1, 1]: 255 against 256, "class3_is_text" on "kinds_stretch_4" at n_wg.  The
variants live on the reference's side only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import chain_task_cases as cc
from test_gpu_chain_stretch import consistent

pytestmark = pytest.mark.gpu

PROBE = os.path.join(os.path.dirname(__file__), "chain_task_probe.py")


def probe(case):
    r = subprocess.run([sys.executable, PROBE], env=cc.environment(case, dict(os.environ, CHAIN_TASK_CASE=case)),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])       # (a mismatch with the oracle ends the probe with 1)
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("case", list(cc.CASES))
def test_task_setup(case):
    name = cc.CASES[case][0]
    d, lays, want = cc.data(name), cc.layouts(name), cc.reference(case)
    out = probe(case)
    # what the set-up is made from: a difference here is k_rowscan's or k_mkdesc's (test_gpu_dp_rows.py)
    for b, (rows, lay) in enumerate(zip(out["rows"], lays)):
        for field in ("kend", "shortcut", "run_row", "winflag"):
            g, w = np.asarray(rows[field], dtype=np.int64), lay[field].astype(np.int64)
            assert g.shape == w.shape and np.array_equal(g, w), f"block {b}: {field} differs first at {int(np.flatnonzero(g != w)[0])}"
    got = {k: (out[k] if isinstance(out[k], int) else np.asarray(out[k], dtype=np.uint32)) for k in
           ("tasks", "task_off", "merged", "kind", "wg_tasks", "wg_desc", "n_wg", "n_wg_runs")}
    got["tasks"], got["wg_desc"] = got["tasks"].reshape(-1, 4), got["wg_desc"].reshape(-1, 2)
    assert cc.invariants(got, d.sizes, lays, cc.knobs(case)) is None
    assert cc.first_difference(got, want) is None
    # the tasks the device starts at a cut point (the quality pin of the text case: all but one at the most)
    at_cut = lambda ct: sum(1 for b, q, pout, _ in ct["tasks"].astype(int).tolist()       # noqa: E731
                            if pout and cc.is_cut_brute(lays[b]["kend"], q))
    assert at_cut(got) == at_cut(want)
    st = dict(out["stats"], blocks=out["blocks"])
    assert consistent(st), st
    # (three runs; the one task of an empty block has nothing to walk and is not counted: test_stretch_edges)
    assert st["tasks"] == 3 * (len(want["tasks"]) - sum(1 for B in d.sizes if B == 0)), st
