"""Run by tests/test_gpu_chain_tasks.py in a subprocess (the knobs of the chain's task set-up are read from the
environment once per process): one case of chain_task_cases.py, named by CHAIN_TASK_CASE.  Builds the tables, reads back
the DP row fields the set-up is made from (Tables.dp_rows of every block) and the set-up itself (Tables.chain_tasks),
then runs the three chained squeeze runs of chain_stretch_probe.py against the CPU oracle.  One JSON line: the arrays,
zmx_last_seg_stats and the digest."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import chain_stretch_probe as sp  # noqa: E402
import chain_task_cases as cc  # noqa: E402
from zopfli_amd import Context, api  # noqa: E402


def main():
    d = cc.data(cc.CASES[os.environ["CHAIN_TASK_CASE"]][0])
    lib = api.library()
    ctx = Context(0, lib)
    ctx.set_input(d.data)
    t = ctx.build_tables(d.blocks)
    rows = []
    for b in range(len(d.blocks)):
        r = t.dp_rows(b)
        rows.append({name: r[name].tolist() for name in ("kend", "shortcut", "run_row", "winflag")})
    ct = t.chain_tasks()
    out = {name: (v if isinstance(v, int) else v.tolist()) for name, v in ct.items()}
    out["rows"] = rows
    out["digest"] = sp.squeeze_runs_against_oracle(t, d.data, d.blocks)
    t.free()
    ctx.close()
    out["stats"] = api.last_seg_stats(lib)
    out["blocks"] = sum(1 for (s, e) in d.blocks if e > s)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
