"""Writes tests/golden/png_decode.json: what the real LodePNG makes of the cases of tests/png_decode_cases.py.  Needs the
reference's tree (REF, default as in oracle/Makefile); tools/models/png_decode_model.cc is compiled against it in a
temporary directory.
  valid      name -> "file_sha256" (the case's file: the writer is byte-stable), "own" and "rgba8": the SHA-256 of LodePNG's
             pixels from lodepng_decode without colour conversion and from lodepng_decode32.  Below 8 bits LodePNG packs
             the own-mode rows bit after bit with no padding at a row's end; the library's layout is rows of whole bytes
             with the padding bits zero (zmx_png_index_image.d_pixels).  The hash is taken after re-padding: the first
             width * bitdepth bits of every row, then zero bits up to the next whole byte.
  malformed  name -> "file" (hex) and "error": LodePNG's error number (of lodepng_decode; lodepng_decode32 must agree on
             whether there is one).  A valid case LodePNG refuses for an ancillary chunk it reads and the library skips
             (png_decode_cases.LODEPNG_REFUSES) has "error" in place of the hashes.  The valid interlaced file has error 0: the library recognises and refuses it.
The JSON holds data only.  Run from the repository root: python tests/golden/make_png_decode_golden.py"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import png_decode_cases as pc  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
LODEPNG_DIR = os.environ.get("LODEPNG_DIR", os.path.join(REF, "src", "zopflipng", "lodepng"))
GOLDEN = os.path.join(ROOT, "tests", "golden", "png_decode.json")


def repad(packed, width, height, bpp):
    """LodePNG's bit-packed rows as rows of whole bytes, the padding bits zero"""
    if bpp >= 8 or (width * bpp) % 8 == 0:
        return packed
    bits = "".join(f"{b:08b}" for b in packed)
    line = width * bpp
    out = bytearray()
    for r in range(height):
        row = bits[r * line:(r + 1) * line]
        row += "0" * (-len(row) % 8)
        out += bytes(int(row[i:i + 8], 2) for i in range(0, len(row), 8))
    return bytes(out)


def main():
    valid = pc.valid_cases()
    bad = pc.malformed_cases() + pc.truncation_cases()
    out = {"valid": {}, "malformed": {}}
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "png_decode_model")
        subprocess.check_call(["g++", "-O2", "-w", "-I", LODEPNG_DIR, os.path.join(ROOT, "tools", "models", "png_decode_model.cc"),
                               os.path.join(LODEPNG_DIR, "lodepng.cpp"), "-o", exe])
        text = "".join((c.file.hex() or "-") + "\n" for c in valid + bad)
        lines = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == len(valid) + len(bad)
    for case, line in zip(valid, lines):
        error, w, h, ct, bd, own, error32, rgba = line.split()
        if case.name in pc.LODEPNG_REFUSES:      # (the stated exception: LodePNG reads the ancillary chunks it knows)
            assert int(error) == int(error32) == pc.LODEPNG_REFUSES[case.name], (case.name, error, error32)
            out["valid"][case.name] = {"file_sha256": hashlib.sha256(case.file).hexdigest(), "error": int(error)}
            continue
        assert error == "0" and error32 == "0", (case.name, error, error32)
        own = repad(bytes.fromhex(own), int(w), int(h), pc.bpp_of(int(ct), int(bd)))
        out["valid"][case.name] = {"file_sha256": hashlib.sha256(case.file).hexdigest(), "own": hashlib.sha256(own).hexdigest(),
                                   "rgba8": hashlib.sha256(bytes.fromhex(rgba)).hexdigest()}
    for b, line in zip(bad, lines[len(valid):]):
        error, _, _, _, _, _, error32, _ = line.split()
        assert (error == "0") == (error32 == "0"), (b.name, error, error32)
        out["malformed"][b.name] = {"file": b.file.hex(), "error": int(error)}
        print(b.name, error)
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
