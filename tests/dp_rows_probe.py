"""Run by tests/test_gpu_dp_rows.py in a subprocess (ZOPFLI_AMD_RUN_CODES is read once per process): every case of
dp_row_cases.py through Tables.dp_rows against reference_layout, with or without codeless rows as the environment
says, then one JSON line: {"codeless", "cases", "blocks", "codeless_rows", "diff"}, diff = the first difference or null."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import dp_row_cases as dc  # noqa: E402
from zopfli_amd import Context, api  # noqa: E402


def compare_case(ctx, name, codeless, parent_blocks=None):
    """The first difference between the device's layout of a case and the reference's, as text naming the block, or
    None.  parent_blocks: the tables are built from matches-only tables over those blocks (zmx_tables_build_from)."""
    c = dc.case(name)
    want = dc.layouts(name, codeless)
    ctx.set_input(c.data)
    pt = ctx.build_tables(parent_blocks, matches_only=True) if parent_blocks else None
    t = None
    try:
        t = ctx.build_tables(c.blocks, parent=pt)
        for b in range(len(c.blocks)):
            diff = dc.first_difference(t.dp_rows(b), want[b])
            if diff:
                return f"case {name}, block {b} {c.blocks[b]}: {diff}"
    finally:
        if t is not None:
            t.free()
        if pt is not None:
            pt.free()
    return None


def main():
    codeless = os.environ.get("ZOPFLI_AMD_RUN_CODES", "0") in ("", "0")
    ctx = Context(0, api.library())
    out = dict(codeless=codeless, cases=0, blocks=0, codeless_rows=0, diff=None)
    for name in dc.CASES:
        out["diff"] = compare_case(ctx, name, codeless)
        if out["diff"]:
            break
        out["cases"] += 1
        out["blocks"] += len(dc.case(name).blocks)
        out["codeless_rows"] += int(sum(int(lay["codeless"].sum()) for lay in dc.layouts(name, codeless)))
    ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
