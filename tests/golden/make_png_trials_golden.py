"""Writes tests/golden/png_trials.json: what the real LodePNG and the real zopflipng make of the cases of
tests/png_trial_cases.py.  Needs the reference's tree (REF, default as in oracle/Makefile) and oracle/_ref built from it.
  buffers     name -> lodepng_zlib_compress' length at window 8192 (tools/models/png_lodeflate_model.cc `size`; the model's
              own figure beside it must agree)
  histograms  name -> the same with use_lz77 0 (`huff`): the dynamic trees alone
  images      "name|keepcolortype|lossy_transparent|types" -> the eight trial file sizes of zopflipng's
              AutoChooseFilterStrategy and the index it takes (tools/models/png_trials_model.cc, which calls zopflipng's
              own TryOptimize); the choice is held against the file oracle/_ref/zopflipng_ref writes without --filters,
              which must be the one it writes with the chosen strategy.
Run from the repository root: python tests/golden/make_png_trials_golden.py"""
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import png_encode_cases as ec  # noqa: E402
import png_trial_cases as tc  # noqa: E402
from png_rows_cases import filter_rows  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
PNGSRC = os.path.join(REF, "src", "zopflipng")
LODEPNG_DIR = os.environ.get("LODEPNG_DIR", os.path.join(PNGSRC, "lodepng"))
PNG_REF = os.path.join(ROOT, "oracle", "_ref", "zopflipng_ref")
LETTERS = ["0", "1", "2", "3", "4", "m", "e", "p"]


def build(tmp):
    lo = os.path.join(tmp, "png_lodeflate_model")
    tr = os.path.join(tmp, "png_trials_model")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-I", LODEPNG_DIR, "-I", os.path.join(ROOT, "zopfli_amd", "csrc", "host"),
                           os.path.join(ROOT, "tools", "models", "png_lodeflate_model.cc"), "-o", lo])
    objs = sorted(glob.glob(os.path.join(ROOT, "oracle", "_ref", "zref_obj", "*.o")))
    assert objs, "oracle/_ref is not built"
    subprocess.check_call(["g++", "-O2", "-w", "-I", PNGSRC, os.path.join(ROOT, "tools", "models", "png_trials_model.cc"),
                           os.path.join(PNGSRC, "zopflipng_lib.cc"), os.path.join(LODEPNG_DIR, "lodepng.cpp"),
                           os.path.join(LODEPNG_DIR, "lodepng_util.cpp")] + objs + ["-lm", "-o", tr])
    return lo, tr


def input_png(name, types):
    nm, w, h, ct, depth = tc.image_case(name)
    bw = ec.CHANNELS[ct] * depth // 8
    return ec.plain_png((w, h, ct, depth), filter_rows(tc.image(name), bw, types))


def main():
    out = {"window": tc.WINDOW, "buffers": {}, "histograms": {}, "images": {}}
    with tempfile.TemporaryDirectory() as tmp:
        lo, tr = build(tmp)
        path = os.path.join(tmp, "buf.bin")
        for name in tc.BUFFER_IDS:
            tc.buffer(name).tofile(path)
            lode, model = (int(v) for v in subprocess.check_output([lo, "size", path, str(tc.WINDOW)]).split())
            assert lode == model, (name, lode, model)
            out["buffers"][name] = lode
        for name in tc.HIST_IDS:
            tc.hist_buffer(name).tofile(path)
            lode, model = (int(v) for v in subprocess.check_output([lo, "huff", path]).split())
            assert lode == model, (name, lode, model)
            out["histograms"][name] = lode
        runs = []
        for name in tc.IMAGE_IDS:
            for keep in (1, 0):
                runs.append((name, keep, 0, None))
            if tc.image_case(name)[3] in (4, 6) and tc.image_case(name)[4] == 8:
                runs.append((name, 1, 1, None))
                runs.append((name, 0, 1, None))
        for label, (name, types) in tc.PREDEFINED_RUNS.items():
            runs.append((name, 1, 0, label))
            runs.append((name, 0, 0, label))
        src, dst = os.path.join(tmp, "in.png"), os.path.join(tmp, "out.png")
        for name, keep, lossy, label in runs:
            h = tc.image_case(name)[2]
            types = np.zeros(h, dtype=np.uint8) if label is None else tc.PREDEFINED_RUNS[label][1](h)
            with open(src, "wb") as f:
                f.write(input_png(name, types))
            vals = [int(v) for v in subprocess.check_output([tr, src, str(keep), str(lossy), "0"]).split()]
            sizes, best = vals[:8], vals[8]
            # the choice, as zopflipng itself makes it
            flags = ["-y", "--always_zopflify", "--iterations=2"] + (["--keepcolortype"] if keep else []) + (["--lossy_transparent"] if lossy else [])
            subprocess.check_call([PNG_REF] + flags + [src, dst], stdout=subprocess.DEVNULL)
            with open(dst, "rb") as f:
                auto = f.read()
            subprocess.check_call([PNG_REF] + flags + ["--filters=" + LETTERS[best], src, dst], stdout=subprocess.DEVNULL)
            with open(dst, "rb") as f:
                assert f.read() == auto, (name, keep, lossy, label, best)
            out["images"]["|".join([name, str(keep), str(lossy), label or "-"])] = {"sizes": sizes, "best": best}
            print(name, keep, lossy, label, sizes, LETTERS[best])
    with open(tc.GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
