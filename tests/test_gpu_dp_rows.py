"""The DP row layout of the table build — dph[] (k_rowscan), codes[] (k_codes), wmeta[] / winflag[] / winroff[]
(k_mkdesc) — read back with Tables.dp_rows (zmx_dp_rows_download) and held to the plain reference of dp_row_cases.py, on
the cases of that file, which stand on the kernels' edges (what they reach is asserted without a GPU in
test_cpu_dp_row_cases.py, where the reference itself is held to the oracle's GetBestLengths).  The squeeze runs show
these arrays only through the paths that win; here every row, every edge's code and every window word of every block
is compared.  Integer equality, no tolerance; words 35..39 of a window record, codes past block_edges and the records of
an empty block are not defined and not compared."""
import json
import os
import subprocess
import sys

import pytest

import dp_row_cases as dc
import dp_rows_probe as probe

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", dc.CASES)
def test_layout_equals_reference(gpu_ctx, name):
    """The default layout (wide run rows without codes), in this process."""
    diff = probe.compare_case(gpu_ctx, name, codeless=True)
    assert diff is None, diff


def test_layout_from_parent_tables(gpu_ctx):
    """The multi-block case built from matches-only tables over the enclosing range: the records are copied
    (k_copy_recs), only the block ends are computed again — the layout is the same arrays."""
    diff = probe.compare_case(gpu_ctx, "multi", codeless=True, parent_blocks=dc.MULTI_PARENT)
    assert diff is None, diff


def test_layout_with_codes_for_every_row():
    """ZOPFLI_AMD_RUN_CODES=1 (read once per process: a child runs dp_rows_probe.py): every case equals the reference
    built without codeless rows, and no row is codeless — of the more than 100 000 rows that are in the default layout
    of the same cases."""
    script = os.path.join(os.path.dirname(__file__), "dp_rows_probe.py")
    r = subprocess.run([sys.executable, script], env=dict(os.environ, ZOPFLI_AMD_RUN_CODES="1"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    st = json.loads(r.stdout.strip().splitlines()[-1])
    assert st["diff"] is None, st["diff"]
    assert st["codeless"] is False and st["codeless_rows"] == 0 and st["cases"] == len(dc.CASES), st
    assert sum(int(lay["codeless"].sum()) for name in dc.CASES for lay in dc.layouts(name, True)) > 100000
