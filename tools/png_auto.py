"""zopflipng's automatic filter-strategy choice on an image in device memory: what the kernels of
zmx_png_deflate_sizes_device cost, what ZMX_PNG_FILTER_AUTO costs on top of the encode it chooses for, and what the entries
cost those who do not ask.

Four tables, each measured in a child process of its own; inside a process the ways that are compared alternate, after a
warm-up call of each, and a line gives the best of --repeat runs and the spread (max - min).
(a) the six kernels alone, by HIP events (zmx_internal_png_lodeflate_ms), on the eight trials' scanlines (types 0 .. 4,
    minimum sum, entropy, and entropy again in the predefined trial's place) of a --size x --size RGBA8 photograph-like
    image in ONE call, and on those of --icons icons of 64 x 64 in ONE call; ms and positions/s (input bytes) per kernel.
(b) zmx_png_encode_device(AUTO) against zmx_png_encode_device(<the strategy it chose>), numiterations 5: the difference
    is what the choice costs (the trial rows, the six kernels, the host's trees).
(c) for information: oracle/_ref/zopflipng_amd2 -y --always_zopflify --keepcolortype on the same image as a file (its
    trials run LodePNG on host threads), where it was built.
(d) zmx_png_encode_device(ENTROPY) against the library at --parent-lib where one is given (the build of the commit
    before), else this library twice.  It may not be slower by more than the two spreads together.

usage: python tools/png_auto.py [--repeat 5] [--size 4096] [--icons 1000] [--parent-lib PATH]
prints the tables and one JSON line
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from png_device import _alternate, _image, _stats  # noqa: E402
from png_lossy import _icons  # noqa: E402

KERNELS = ["k_png_lo_hash", "k_png_lo_links", "k_png_lo_ask", "k_png_lo_keep", "k_png_lo_search", "k_png_lo_parse"]
TRIALS = [0, 1, 2, 3, 4, 5, 6, 6]


def _trial_rows(ctx, torch, images):
    """The scanlines of the eight trials of every (H, W, 4) uint8 device image, back to back in one buffer: (buffer, ranges)."""
    total = sum(8 * im.shape[0] * (im.shape[1] * 4 + 1) for im in images)
    rows = torch.empty(total, dtype=torch.uint8, device="cuda")
    at, ranges = 0, []
    for im in images:
        h, n = im.shape[0], im.shape[1] * 4
        types = torch.empty(h, dtype=torch.uint8, device="cuda")
        for strategy in TRIALS:
            ctx.png_filter_types_device(im, n, h, 4, strategy, types)
            ctx.png_filter_rows_device(im, n, h, 4, types, rows.data_ptr() + at, h * (n + 1))
            ranges.append((rows.data_ptr() + at, h * (n + 1)))
            at += h * (n + 1)
    return rows, ranges


def _kernels(args):
    import torch

    from zopfli_amd import Context, api
    lib = api.library()
    lib.zmx_internal_png_lodeflate_ms.argtypes = [ctypes.POINTER(ctypes.c_double)]
    lib.zmx_internal_png_lodeflate_ms.restype = None
    lib.zmx_set_kernel_timing(1)
    ctx = Context(0, lib)
    out = {}
    sets = {f"{args.size} x {args.size} RGBA8, 8 trials": [torch.from_numpy(_image(args.size)).cuda()],
            f"{args.icons} icons of 64 x 64, 8 trials each": [torch.from_numpy(i).cuda() for i in _icons(args.icons)]}
    ms6 = (ctypes.c_double * 6)()
    for name, images in sets.items():
        torch.cuda.synchronize()
        rows, ranges = _trial_rows(ctx, torch, images)
        positions = sum(r[1] for r in ranges)
        runs, wall = [], []
        for i in range(args.repeat + 1):
            t0 = time.perf_counter()
            sizes = ctx.png_deflate_sizes_device(ranges, 8192)
            t1 = time.perf_counter()
            lib.zmx_internal_png_lodeflate_ms(ms6)
            if i:
                runs.append(list(ms6))
                wall.append((t1 - t0) * 1e3)
        rec = {"positions": positions, "buffers": len(ranges), "zlib_bytes": sum(sizes)}
        for k, kernel in enumerate(KERNELS):
            rec[kernel] = _stats([r[k] for r in runs])
            rec[kernel]["Mpos/s"] = round(positions / 1e3 / max(rec[kernel]["best_ms"], 1e-6), 1)
        rec["all six"] = _stats([sum(r) for r in runs])
        rec["all six"]["Mpos/s"] = round(positions / 1e3 / rec["all six"]["best_ms"], 1)
        rec["the call (wall, kernel timing on)"] = _stats(wall)
        out[name] = rec
        del rows
    ctx.close()
    return out


def _choice(args):
    import torch

    from zopfli_amd import Context, ZopfliOptions, api
    lib = api.library()
    d = torch.from_numpy(_image(args.size)).cuda()
    torch.cuda.synchronize()
    ctx = Context(0, lib)
    chosen, trial_sizes = ctx.png_choose_strategy_device(d)
    ctx.close()
    opt = ZopfliOptions(5)
    sizes = {}

    def auto():
        sizes["auto"] = len(api.png_encode_device(d, api.PNG_FILTER_AUTO, opt, lib=lib))

    def fixed():
        sizes["chosen"] = len(api.png_encode_device(d, chosen, opt, lib=lib))

    ms = _alternate({"zmx_png_encode_device(AUTO)": auto, "zmx_png_encode_device(the strategy it chose)": fixed}, args.repeat)
    rec = {k: _stats(v) for k, v in ms.items()}
    rec["difference_ms"] = round(rec["zmx_png_encode_device(AUTO)"]["best_ms"] - rec["zmx_png_encode_device(the strategy it chose)"]["best_ms"], 2)
    rec["chosen"] = chosen
    rec["trial_file_bytes"] = trial_sizes
    rec["bytes"] = sizes
    return rec


def _file_way(args):
    import png_encode_cases as ec
    from png_rows_cases import filter_rows
    exe = os.path.join(ROOT, "oracle", "_ref", "zopflipng_amd2")
    if not os.path.exists(exe):
        return {"built": False}
    import numpy as np
    w = args.size
    img = _image(w).reshape(w, 4 * w)
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = os.path.join(tmp, "in.png"), os.path.join(tmp, "out.png")
        with open(src, "wb") as f:
            f.write(ec.plain_png((w, w, 6, 8), filter_rows(img, 4, np.zeros(w, dtype=np.uint8))))
        ms = []
        for _ in range(2):
            t0 = time.perf_counter()
            subprocess.check_call([exe, "-y", "--always_zopflify", "--keepcolortype", src, dst], stdout=subprocess.DEVNULL)
            ms.append((time.perf_counter() - t0) * 1e3)
        return {"built": True, "zopflipng_amd2 (a process, from a file)": _stats(ms), "bytes": os.path.getsize(dst)}


def _unasked(args):
    import torch

    from zopfli_amd import ZopfliOptions, api
    lib = api.library()
    parent = api.library(args.parent_lib) if args.parent_lib else lib
    d = torch.from_numpy(_image(args.size)).cuda()
    torch.cuda.synchronize()
    opt = ZopfliOptions(5)
    sizes = {}

    def now():
        sizes["now"] = len(api.png_encode_device(d, "e", opt, lib=lib))

    def before():
        sizes["before"] = len(api.png_encode_device(d, "e", opt, lib=parent))

    ms = _alternate({"zmx_png_encode_device(ENTROPY)": now, "zmx_png_encode_device(ENTROPY) (before)": before}, args.repeat)
    rec = {k: _stats(v) for k, v in ms.items()}
    a, b = rec["zmx_png_encode_device(ENTROPY)"], rec["zmx_png_encode_device(ENTROPY) (before)"]
    rec["difference_ms"] = round(a["best_ms"] - b["best_ms"], 2)
    rec["allowed_ms"] = round(a["spread_ms"] + b["spread_ms"], 2)
    rec["bytes"] = sizes
    rec["parent_library"] = bool(args.parent_lib)
    return rec


TABLES = {"kernels": _kernels, "choice": _choice, "file": _file_way, "unasked": _unasked}


def _child(table, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", table, "--repeat", str(args.repeat), "--size", str(args.size),
           "--icons", str(args.icons)] + (["--parent-lib", args.parent_lib] if args.parent_lib else [])
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{table}: {r.stderr[-3000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def _line(name, s, extra=""):
    print(f"  {name:<60}{s['best_ms']:>12.3f}{s['spread_ms']:>11.3f}{extra}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--icons", type=int, default=1000)
    ap.add_argument("--parent-lib", default=None, help="libzopfli_amd.so of the commit before, for table (d)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(TABLES[args.child](args)), flush=True)
        return
    results = {}
    head = f"  {'':<60}{'best ms':>12}{'spread ms':>11}"
    results["kernels"] = ker = _child("kernels", args)
    print(f"(a) the kernels of zmx_png_deflate_sizes_device alone (HIP events), window 8192, best of {args.repeat} after a warm-up")
    for name, rec in ker.items():
        print(f"  {name}: {rec['buffers']} buffers, {rec['positions']} positions, {rec['zlib_bytes']} zlib bytes in all")
        print(head + "     Mpos/s")
        for kernel in KERNELS + ["all six"]:
            _line(kernel, rec[kernel], f"{rec[kernel]['Mpos/s']:>11.1f}")
        _line("the call (wall, kernel timing on)", rec["the call (wall, kernel timing on)"])
    results["choice"] = ch = _child("choice", args)
    print(f"\n(b) {args.size} x {args.size} RGBA8, numiterations 5 (wall, one process, ways alternating); chosen: {ch['chosen']}, "
          f"trial file bytes {ch['trial_file_bytes']}")
    print(head)
    for way in ("zmx_png_encode_device(AUTO)", "zmx_png_encode_device(the strategy it chose)"):
        _line(way, ch[way])
    print(f"    bytes {ch['bytes']};  AUTO - chosen = {ch['difference_ms']} ms: what the choice costs")
    results["file"] = fw = _child("file", args)
    print("\n(c) for information: the file-based library on the same image (two runs)")
    if fw["built"]:
        print(head)
        _line("zopflipng_amd2 (a process, from a file)", fw["zopflipng_amd2 (a process, from a file)"])
        print(f"    bytes {fw['bytes']}")
    else:
        print("    oracle/_ref/zopflipng_amd2 was not built")
    results["unasked"] = un = _child("unasked", args)
    against = "the parent commit's library" if un["parent_library"] else "this library"
    print(f"\n(d) {args.size} x {args.size} RGBA8, strategy e, numiterations 5 (wall, one process, ways alternating); 'before' is {against}'s")
    print(head)
    for way in ("zmx_png_encode_device(ENTROPY)", "zmx_png_encode_device(ENTROPY) (before)"):
        _line(way, un[way])
    print(f"    bytes {un['bytes']}")
    print(f"    now - before = {un['difference_ms']} ms; allowed: both spreads = {un['allowed_ms']} ms: "
          f"{'holds' if un['difference_ms'] <= un['allowed_ms'] else 'DOES NOT HOLD'}")
    print()
    print(json.dumps({"repeat": args.repeat, "size": args.size, "icons": args.icons, "results": results}))


if __name__ == "__main__":
    main()
