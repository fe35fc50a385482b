"""zopflipng's brute-force filter strategy (`--filters=b`) on libzopflipng_amd.so, where LodePNG's per-row search runs on
the device (zmx_png_filter_types_brute, k_png_brute).

  python tools/png_brute.py --make-golden      the all-reference zopflipng on the 1024 x 1024 image of
                                               tools/png_at_size.py with --filters=b --iterations=1, here on the CPU:
                                               input / output SHA-256, size, the 1024 filter-type bytes and its wall
                                               time go to tests/golden/png_brute.json
  python tools/png_brute.py [--runs N] [--exe PATH] [--out FILE]
                                               times zopflipng_amd2 (or PATH, e.g. a parent build) N times (default 3)
                                               on the command lines below and prints one JSON line:
      brute_1024     -y --filters=b --iterations=1   the 1024 x 1024 image
      brute_strip    -y --filters=b --iterations=1   the top 4096 x 256 strip of the 4096 x 4096 image
      default_1024   -y                              the 1024 x 1024 image (the brute search must not run)
"""
import hashlib
import json
import os
import struct
import subprocess
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zopfli_amd._build import PNG_AMD2, PNG_REF  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "png_brute.json")


def _chunk(tag, data):
    body = tag + data
    return struct.pack(">I", len(data)) + body + struct.pack(">I", zlib.crc32(body) & 0xffffffff)


def at_size_pixels(w):
    """tools/png_at_size.py's W x W RGBA image (a gradient with +-3 of noise, seed 7) as an (h, w, 4) array."""
    rng = np.random.default_rng(7)
    y, x = np.mgrid[0:w, 0:w]
    img = np.stack([(x * 255 // max(w - 1, 1)), (y * 255 // max(w - 1, 1)), ((x + y) // 3 % 256),
                    np.full_like(x, 255)], axis=-1).astype(np.int32)
    img[..., :3] += rng.integers(-3, 4, size=(w, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def write_rgba(path, img):
    h, w = img.shape[:2]
    raw = np.concatenate([np.zeros((h, 1), dtype=np.uint8), img.reshape(h, w * 4)], axis=1).tobytes()
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0))
                + _chunk(b"IDAT", zlib.compress(raw, 1)) + _chunk(b"IEND", b""))


def filter_bytes(png):
    """The filter-type byte of every row of a non-interlaced 8-bit-or-more PNG (from its IHDR and IDAT)."""
    pos, idat, w, h, bpp = 8, b"", 0, 0, 0
    while pos < len(png):
        n = struct.unpack(">I", png[pos:pos + 4])[0]
        tag, data = png[pos + 4:pos + 8], png[pos + 8:pos + 8 + n]
        if tag == b"IHDR":
            w, h, depth, ct = struct.unpack(">IIBB", data[:10])
            bpp = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[ct] * depth
        elif tag == b"IDAT":
            idat += data
        pos += 12 + n
    rows = zlib.decompress(idat)
    line = (w * bpp + 7) // 8 + 1
    assert len(rows) == h * line
    return bytes(rows[y * line] for y in range(h))


def make_golden():
    tmp = os.environ.get("TMPDIR", "/tmp")
    src, dst = os.path.join(tmp, "brute_in1024.png"), os.path.join(tmp, "brute_out1024.png")
    write_rgba(src, at_size_pixels(1024))
    t0 = time.perf_counter()
    r = subprocess.run([PNG_REF, "-y", "--filters=b", "--iterations=1", src, dst], capture_output=True, text=True, timeout=20000)
    secs = time.perf_counter() - t0
    assert r.returncode == 0, r.stdout + r.stderr
    with open(src, "rb") as f:
        inp = f.read()
    with open(dst, "rb") as f:
        out = f.read()
    gold = {"1024": {"args": ["-y", "--filters=b", "--iterations=1"], "input_sha256": hashlib.sha256(inp).hexdigest(),
                     "sha256": hashlib.sha256(out).hexdigest(), "bytes": len(out), "filter_types": filter_bytes(out).hex(),
                     "reference_seconds_here": round(secs, 1)}}
    with open(GOLDEN, "w") as f:
        json.dump(gold, f, indent=1)
    print(json.dumps({k: v for k, v in gold["1024"].items() if k != "filter_types"}), flush=True)


def main():
    if "--make-golden" in sys.argv:
        make_golden()
        return
    runs = int(sys.argv[sys.argv.index("--runs") + 1]) if "--runs" in sys.argv else 3
    exe = sys.argv[sys.argv.index("--exe") + 1] if "--exe" in sys.argv else PNG_AMD2
    tmp = os.environ.get("TMPDIR", "/tmp")
    big = at_size_pixels(4096)
    images = {"1024": at_size_pixels(1024), "strip": big[:256]}
    res = {"exe": os.path.relpath(exe, ROOT), "runs": runs}
    for name, img, args in (("brute_1024", "1024", ["--filters=b", "--iterations=1"]),
                            ("brute_strip", "strip", ["--filters=b", "--iterations=1"]),
                            ("default_1024", "1024", [])):
        src, dst = os.path.join(tmp, f"pb_in_{img}.png"), os.path.join(tmp, f"pb_out_{name}.png")
        write_rgba(src, images[img])
        secs, shas = [], set()
        for _ in range(runs):
            t0 = time.perf_counter()
            r = subprocess.run([exe, "-y"] + args + [src, dst], capture_output=True, text=True, timeout=3000)
            secs.append(round(time.perf_counter() - t0, 3))
            if r.returncode != 0:
                res[name + "_err"] = (r.stdout + r.stderr)[-500:]
                break
            with open(dst, "rb") as f:
                shas.add(hashlib.sha256(f.read()).hexdigest())
        res[name] = {"seconds": secs, "median": sorted(secs)[len(secs) // 2], "sha256": sorted(shas)}
    line = json.dumps(res)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "a") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
