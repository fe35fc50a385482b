"""Writes tests/golden/png_sink.json: what the real lodepng_convert makes of the files of tests/png_sink_cases.py
(all_files()).  Needs the reference's tree (REF, default as in oracle/Makefile); tools/models/png_sink_model.cc is compiled
against it in a temporary directory.
  name -> "file_sha256" (the case's file: the writer is byte-stable) and "c<channels>_d<depth>" for channels 1 .. 4 (grey,
  grey + alpha, RGB, RGBA) and depth 8, 16: the SHA-256 of lodepng_convert's image from the file's own mode into that one,
  16-bit samples high byte first.
The JSON holds data only.  Run from the repository root: python tests/golden/make_png_sink_golden.py"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import png_sink_cases as sk  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
LODEPNG_DIR = os.environ.get("LODEPNG_DIR", os.path.join(REF, "src", "zopflipng", "lodepng"))
GOLDEN = os.path.join(ROOT, "tests", "golden", "png_sink.json")


def main():
    files = sk.all_files()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "png_sink_model")
        subprocess.check_call(["g++", "-O2", "-w", "-I", LODEPNG_DIR, os.path.join(ROOT, "tools", "models", "png_sink_model.cc"),
                               os.path.join(LODEPNG_DIR, "lodepng.cpp"), "-o", exe])
        text = "".join(f.file.hex() + "\n" for f in files)
        lines = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == len(files)
    for f, line in zip(files, lines):
        fields = line.split()
        m, _ = sk.mode_of(f.file)
        assert fields[0] == "0" and (int(fields[1]), int(fields[2])) == (m["width"], m["height"]), (f.name, fields[:3])
        entry = {"file_sha256": hashlib.sha256(f.file).hexdigest()}
        for k, (channels, depth) in enumerate(sk.MODES):
            error, image = fields[3 + 2 * k], fields[4 + 2 * k]
            assert error == "0", (f.name, channels, depth, error)
            assert len(image) == 2 * m["width"] * m["height"] * channels * depth // 8
            entry[f"c{channels}_d{depth}"] = hashlib.sha256(bytes.fromhex(image)).hexdigest()
        out[f.name] = entry
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
