"""Writes tests/golden/png_index.json: the files the all-reference zopflipng (oracle/_ref/zopflipng_ref, built from the
reference's tree by oracle/Makefile) writes for the small cases of tests/png_index_cases.py, as hex:
  files["<case>|keep|<filters>|<lossy>"]      zopflipng --keepcolortype --always_zopflify --iterations=2 --filters=<f> [--lossy_transparent]
  files["<case>|optimize|<filters>|<lossy>"]  the same without --keepcolortype
<filters> is 0, or "auto" (no --filters) for png_index_cases.GOLDEN_AUTO.  CPU only.
Run from the repository root: python tests/golden/make_png_index_golden.py"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import png_index_cases as ic  # noqa: E402
from zopfli_amd._build import PNG_REF  # noqa: E402

ITERATIONS = 2
OUT = os.path.join(ROOT, "tests", "golden", "png_index.json")


def reference(tmp, case, filters, keep, lossy):
    """zopflipng_ref's file for the case written as a palette or low-bit grey PNG."""
    src, dst = os.path.join(tmp, "in.png"), os.path.join(tmp, "ref.png")
    with open(src, "wb") as f:
        f.write(ic.input_png(case))
    flags = ["-y", "--always_zopflify", f"--iterations={ITERATIONS}"] + ([] if filters == "auto" else [f"--filters={filters}"]) + \
        (["--keepcolortype"] if keep else []) + (["--lossy_transparent"] if lossy else [])
    r = subprocess.run([PNG_REF] + flags + [src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-1000:])
    with open(dst, "rb") as f:
        return f.read()


def main():
    files = {}
    with tempfile.TemporaryDirectory() as tmp:
        for case in ic.SMALL:
            for filters in ["0"] + (["auto"] if case[0] in ic.GOLDEN_AUTO else []):
                for keep in (True, False):
                    for lossy in (0, 1):
                        files[f"{case[0]}|{'keep' if keep else 'optimize'}|{filters}|{lossy}"] = reference(tmp, case, filters, keep, lossy).hex()
    with open(OUT, "w") as f:
        json.dump({"iterations": ITERATIONS, "files": files}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(files), "files,", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
