"""Match edges BELOW mincost in the squeeze on the device: k_wtab's list of weights below the run's mincost, k_badscan's
bitmap of the positions that own one (both branches: rows with weight codes, and wide run rows without), the generic
path k_dp5_spec / k_dp4_fix / d3_load_group send such positions down, and the bitmap's state from run to run
(zmx_squeeze_run's badpos_clean, k_badscan's early return for a block without such weights).  Entropy, fixed and dyadic
models with mincost = GetCostModelMinCost never get there; the cases of steer_cases.py do, and
test_cpu_steer_cases.py asserts that on the CPU.  Everything is held to the CPU oracle, which runs squeeze.c:293's test
costs[j + k] <= mincost + costs[j] literally with the mincost it is given.  Integer equality, no tolerance."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import steer_cases as sc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", [c[0] for c in sc.INFLATED])
def test_inflated_mincost(gpu_ctx, name):
    """mincost = GetCostModelMinCost + delta handed to the device and to the oracle alike: length array, store and
    histogram are equal, on every class and block shape of steer_cases.INFLATED (the oracle's result differs from the
    one for the true mincost in every block of real size, so a kernel that skipped the test — or k_badscan — fails)."""
    c = sc.inflated(name)
    gpu_ctx.set_input(c["data"])
    t = gpu_ctx.build_tables(c["blocks"])
    try:
        nb = len(c["blocks"])
        t.greedy(0)
        nsym, hist = t.squeeze_run(c["cost"], c["mincost"], np.ones(nb, dtype=np.int32))
        sc.assert_run_equals_oracle(t, c["blocks"], 1, nsym, hist, c["runs"], name + " inflated")
        # and the same tables with the true mincost again, into the other slot (the bitmap of the run before is stale)
        nsym, hist = t.squeeze_run(c["cost"], c["mincost_true"], np.zeros(nb, dtype=np.int32))
        sc.assert_run_equals_oracle(t, c["blocks"], 0, nsym, hist, c["runs_true"], name + " true")
    finally:
        t.free()


@pytest.mark.parametrize("name", [c[0] for c in sc.ROUNDING])
def test_weight_below_mincost_by_rounding(gpu_ctx, name):
    """A model whose GetCostModelMinCost (1.25) lies above one of its own match weights (1.25 - 2^-52): the documented
    contract of zmx_squeeze_run, and k_badscan runs.  The oracle's parse equals its own for mincost 0 on these models, so
    this leg shows that the flagged positions' generic path is exact, not that the test is honoured (test_inflated_mincost)."""
    c = sc.rounding(name)
    gpu_ctx.set_input(c["data"])
    t = gpu_ctx.build_tables(c["blocks"])
    try:
        nb = len(c["blocks"])
        t.greedy(0)
        nsym, hist = t.squeeze_run(c["cost"], c["mincost"], np.ones(nb, dtype=np.int32))
        sc.assert_run_equals_oracle(t, c["blocks"], 1, nsym, hist, c["runs"], name + " rounding")
    finally:
        t.free()


def test_state_across_runs(gpu_ctx):
    """One table set, five runs in alternating slots: clean, weights below mincost in every block, clean, weights below
    mincost in ONE block of three (mincost is per block), clean.  Each equals the oracle: a bitmap left over from a run
    before, a memset skipped wrongly or a block scanned with another block's list would show."""
    c = sc.state_runs()
    gpu_ctx.set_input(c["data"])
    t = gpu_ctx.build_tables(c["blocks"])
    try:
        nb = len(c["blocks"])
        t.greedy(0)
        for it, (mincost, runs) in enumerate(c["runs"]):
            slot = (it + 1) & 1
            nsym, hist = t.squeeze_run(c["cost"], mincost, np.full(nb, slot, dtype=np.int32))
            sc.assert_run_equals_oracle(t, c["blocks"], slot, nsym, hist, runs, f"run {it} (delta {sc.STATE_RUNS[it]})")
    finally:
        t.free()


# (environment, what the task statistics must show): as test_gpu_parity.CHAIN_ENVS, on seg_probe.py's SEG_PROBE_MINCOST cases
MINCOST_ENVS = [
    ({}, lambda st: st["tasks"] > 0 and st["accepted"] > 0),
    ({"ZOPFLI_AMD_INT_PATH": "0"}, lambda st: st["accepted"] > 0),          # every window in the reference's doubles
    ({"ZOPFLI_AMD_SEG_L": "0"}, lambda st: st["tasks"] == 0),               # the serial chain (k_dp4_fix alone)
    ({"ZOPFLI_AMD_FIX_LEAN": "0"}, lambda st: st["tasks"] > 0),              # serial re-runs by the lean one-wave job
    ({"ZOPFLI_AMD_RUN_CODES": "1"}, lambda st: st["accepted"] > 0),         # run rows WITH codes: k_badscan's other branch sees them
]


@pytest.mark.parametrize("env,expect", MINCOST_ENVS, ids=lambda v: ("-".join(f"{k[11:]}{x}" for k, x in v.items()) or "default") if isinstance(v, dict) else "")
def test_inflated_mincost_through_task_paths(env, expect):
    """seg_probe.py with SEG_PROBE_MINCOST=3 (class T with delta 3, class Z — long runs, rows without codes — with delta
    10; two chained runs each) in a fresh process per task geometry: any mismatch with the oracle fails it."""
    probe = os.path.join(os.path.dirname(__file__), "seg_probe.py")
    r = subprocess.run([sys.executable, probe], env=dict(os.environ, SEG_PROBE_MINCOST="3", **env), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    st = json.loads(r.stdout.strip().splitlines()[-1])
    assert expect(st), st
