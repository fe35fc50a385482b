"""Palette, 1/2/4-bit grey and index images in device memory: what k_png_index_use and k_png_index_convert cost, what the
zmx_png_index_* entries save a caller who today expands to RGBA8 first, and what the generalised strategy trials cost the
entries that were there before.

Three tables, each measured in a child process of its own; inside a process the ways that are compared alternate, after a
warm-up call of each, and a line gives the best of --repeat runs and the spread (max - min).
(a) the two kernels alone, by HIP events (zmx_internal_png_index_ms), on a 4096 x 4096 image: 8 bits over 21 labels in
    large regions; 8 bits over 256 labels as noise (the worst case for the LDS table: every pixel another slot); a 1-bit
    mask.  k_png_index_convert into the image's own mode (a palette of the same depth) and into RGBA at 8 bits.  Each beside
    one hipMemcpyAsync device to device of the same bytes.  GB/s counts the algorithmic bytes: the image read once by
    k_png_index_use; the image read and the output written once by k_png_index_convert; read and written by the copy.
(b) the call against what a caller must do today: `palette[indices]` by torch on the device (for the masks: the bits
    unpacked first) and zmx_png_optimize_device[_batch] of the library at --parent-lib (the build of the commit before; else
    of this library), against zmx_png_index_optimize_device[_batch].  The 4096 x 4096 label map at numiterations 5, strategy
    e; --masks masks of 64 x 64 at 1 bit through the batch at numiterations 15.  The files must be equal, and the new
    entry may not be slower than the baseline by more than the two spreads together.
(c) for information, zmx_png_optimize_device of this library against the parent's on a 4096 x 4096 RGBA8 image under "auto":
    the trials (TrialFileSizes, ChooseStrategy) were generalised.  The difference must stay within the two spreads.

usage: python tools/png_index.py [--repeat 5] [--size 4096] [--masks 1000] [--parent-lib PATH]
prints the tables and one JSON line
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from png_device import _alternate, _image, _stats  # noqa: E402


def _palette(n, seed=5):
    import numpy as np
    pal = np.random.default_rng(seed).integers(0, 256, size=(n, 4), dtype=np.uint8)
    pal[:, 3] = 255
    pal[:, 0] = np.arange(n)   # (distinct colours)
    return pal


def _labels21(w):
    """21 labels in large regions: a segmentation map."""
    import numpy as np
    y, x = np.mgrid[0:w, 0:w]
    return (((x // (w // 7)) + 3 * (y // (w // 5)) + ((x + y) // (w // 3))) % 21).astype(np.uint8)


def _noise256(w):
    import numpy as np
    return np.random.default_rng(3).integers(0, 256, size=(w, w), dtype=np.uint8)


def _mask1(w):
    """A 1-bit mask, packed: discs on a grid."""
    import numpy as np
    y, x = np.mgrid[0:w, 0:w]
    return np.packbits((((x % 256) - 128) ** 2 + ((y % 256) - 128) ** 2 < 90 ** 2).astype(np.uint8), axis=1)


def _masks(k, iw=64):
    import numpy as np
    out = []
    for i in range(k):
        rng = np.random.default_rng(500 + i)
        y, x = np.mgrid[0:iw, 0:iw]
        cx, cy, r = rng.integers(16, 48), rng.integers(16, 48), rng.integers(6, 30)
        out.append(np.packbits(((x - cx) ** 2 + (y - cy) ** 2 < r * r).astype(np.uint8), axis=1))
    return out


BW = [(0, 0, 0, 255), (255, 255, 255, 255)]


def _parent(args, lib):
    from zopfli_amd import api
    if not args.parent_lib:
        return lib
    parent = api.bind(ctypes.CDLL(os.path.abspath(args.parent_lib)))
    parent.zmx_set_kernel_timing(0)
    return parent


def _kernels(args):
    import torch

    from batch_files import _Hip
    from zopfli_amd import Context, api
    lib = api.library()
    lib.zmx_internal_png_index_ms.argtypes = [ctypes.POINTER(ctypes.c_double)]
    lib.zmx_internal_png_index_ms.restype = None
    lib.zmx_set_kernel_timing(1)
    hip = _Hip()
    ctx = Context(0, lib)
    w = args.size
    ms2 = (ctypes.c_double * 2)()
    spare = torch.empty(4 * w * w, dtype=torch.uint8, device="cuda")
    out_buf = torch.empty(4 * w * w, dtype=torch.uint8, device="cuda")
    out = {}
    for name, arr, depth, pal in (("8 bits, 21 labels in regions", _labels21(w), 8, _palette(21)), ("8 bits, 256 labels as noise", _noise256(w), 8, _palette(256)),
                                  ("1-bit mask", _mask1(w), 1, BW)):
        d = torch.from_numpy(arr).cuda()
        torch.cuda.synchronize()
        nbytes = arr.size
        image = (d, w, w, 3, depth, pal)
        first = ctx.png_index_use_device(image)
        own, own_table = api.png_index_keep_plan(image, first, lib=lib)
        rgba = api.PngColorMode()
        rgba.colortype, rgba.bitdepth = 6, 8
        rgba_table = api.png_index_table(image, first, rgba, lib=lib)
        runs = []
        for i in range(args.repeat + 1):
            ctx.png_index_use_device(image)
            lib.zmx_internal_png_index_ms(ms2)
            use = ms2[0]
            ctx.png_index_convert_device(image, own, own_table, out_buf.data_ptr(), nbytes)
            lib.zmx_internal_png_index_ms(ms2)
            conv_own = ms2[1]
            ctx.png_index_convert_device(image, rgba, rgba_table, out_buf.data_ptr(), 4 * w * w)
            lib.zmx_internal_png_index_ms(ms2)
            conv_rgba = ms2[1]
            copy_in = hip.copies_ms(spare.data_ptr(), [(d.data_ptr(), nbytes)])
            copy_out = hip.copies_ms(spare.data_ptr(), [(out_buf.data_ptr(), 4 * w * w)])
            if i:
                runs.append((use, conv_own, conv_rgba, copy_in, copy_out))
        rec = {}
        for k, (label, moved) in enumerate((("k_png_index_use", nbytes), ("k_png_index_convert, own mode", 2 * nbytes),
                                            ("k_png_index_convert, RGBA8", nbytes + 4 * w * w), ("one hipMemcpyAsync of the image", 2 * nbytes),
                                            ("one hipMemcpyAsync of the RGBA8 rows", 8 * w * w))):
            rec[label] = _stats([r[k] for r in runs])
            rec[label]["GB/s"] = round(moved / 1e6 / rec[label]["best_ms"], 1)
        rec["image_bytes"] = nbytes
        rec["values_used"] = sum(f != 2 ** 64 - 1 for f in first)
        out[name] = rec
        del d
    ctx.close()
    return out


def _unpack_bits(packed, w):
    """(h, w) uint8 0 / 1 of rows packed most significant bit first: what a caller does today, on the device."""
    import torch
    shifts = torch.arange(7, -1, -1, dtype=torch.uint8, device=packed.device)
    return ((packed[:, :, None] >> shifts) & 1).reshape(packed.shape[0], -1)[:, :w].contiguous()


def _calls(args):
    import torch

    from zopfli_amd import ZopfliOptions, api
    lib = api.library()
    lib.zmx_set_kernel_timing(0)
    parent = _parent(args, lib)
    w = args.size
    out = {"parent_library": bool(args.parent_lib)}
    labels = torch.from_numpy(_labels21(w)).cuda()
    pal = _palette(21)
    d_pal = torch.from_numpy(pal).cuda()
    torch.cuda.synchronize()
    opt = ZopfliOptions(5)
    got = {}

    def today():
        rgba = d_pal[labels.long()]
        got["today"] = api.png_optimize_device(rgba, "e", opt, lib=parent)

    def new():
        got["new"] = api.png_index_optimize_device(labels, "e", opt, lib=lib, palette=pal)

    ms = _alternate({"zmx_png_index_optimize_device": new, "palette[indices] + zmx_png_optimize_device (before)": today}, args.repeat)
    rec = {k: _stats(v) for k, v in ms.items()}
    rec["files_equal"] = got["new"] == got["today"]
    rec["bytes"] = len(got["new"])
    out["label map"] = rec
    del labels
    masks = [torch.from_numpy(m).cuda() for m in _masks(args.masks)]
    d_bw = torch.tensor(BW, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    opt15 = ZopfliOptions(15)
    images = [(m, 64, 64, 3, 1, BW) for m in masks]

    def batch_today():
        rgba = [d_bw[_unpack_bits(m, 64).long()] for m in masks]
        got["today"] = api.png_optimize_device_batch(rgba, "e", opt15, lib=parent)

    def batch_new():
        got["new"] = api.png_index_optimize_device_batch(images, "e", opt15, lib=lib)

    ms = _alternate({"zmx_png_index_optimize_device_batch": batch_new, "unpack + palette[indices] + zmx_png_optimize_device_batch (before)": batch_today},
                    args.repeat)
    rec = {k: _stats(v) for k, v in ms.items()}
    rec["files_equal"] = got["new"] == got["today"]
    rec["bytes"] = sum(len(f) for f in got["new"])
    out["masks"] = rec
    for rec in (out["label map"], out["masks"]):
        a, b = [rec[k] for k in rec if isinstance(rec[k], dict)]
        rec["difference_ms"] = round(a["best_ms"] - b["best_ms"], 2)
        rec["allowed_ms"] = round(a["spread_ms"] + b["spread_ms"], 2)
    return out


def _existing(args):
    import torch

    from zopfli_amd import ZopfliOptions, api
    lib = api.library()
    lib.zmx_set_kernel_timing(0)
    parent = _parent(args, lib)
    d = torch.from_numpy(_image(args.size)).cuda()
    torch.cuda.synchronize()
    opt = ZopfliOptions(5)
    got = {}

    def now():
        got["now"] = api.png_optimize_device(d, "auto", opt, lib=lib)

    def before():
        got["before"] = api.png_optimize_device(d, "auto", opt, lib=parent)

    ms = _alternate({"zmx_png_optimize_device, auto": now, "zmx_png_optimize_device, auto (before)": before}, args.repeat)
    rec = {k: _stats(v) for k, v in ms.items()}
    a, b = rec["zmx_png_optimize_device, auto"], rec["zmx_png_optimize_device, auto (before)"]
    rec["difference_ms"] = round(a["best_ms"] - b["best_ms"], 2)
    rec["allowed_ms"] = round(a["spread_ms"] + b["spread_ms"], 2)
    rec["files_equal"] = got["now"] == got["before"]
    rec["bytes"] = len(got["now"])
    rec["parent_library"] = bool(args.parent_lib)
    return rec


TABLES = {"kernels": _kernels, "calls": _calls, "existing": _existing}


def _child(table, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", table, "--repeat", str(args.repeat), "--size", str(args.size),
           "--masks", str(args.masks)] + (["--parent-lib", args.parent_lib] if args.parent_lib else [])
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{table}: {r.stderr[-3000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def _line(name, s, extra=""):
    print(f"  {name:<72}{s['best_ms']:>12.3f}{s['spread_ms']:>11.3f}{extra}")


def _verdict(rec, what):
    print(f"    bytes {rec['bytes']}; the files are equal: {rec['files_equal']}")
    print(f"    {what} = {rec['difference_ms']} ms; allowed: both spreads = {rec['allowed_ms']} ms: "
          f"{'holds' if rec['difference_ms'] <= rec['allowed_ms'] else 'DOES NOT HOLD'}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--masks", type=int, default=1000)
    ap.add_argument("--parent-lib", default=None, help="libzopfli_amd.so of the commit before, for tables (b) and (c)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(TABLES[args.child](args)), flush=True)
        return
    results = {}
    head = f"  {'':<72}{'best ms':>12}{'spread ms':>11}"
    results["kernels"] = ker = _child("kernels", args)
    print(f"(a) the kernels alone (HIP events) on {args.size} x {args.size}, best of {args.repeat} after a warm-up")
    print(head + "       GB/s")
    for name, rec in ker.items():
        for label, s in rec.items():
            if isinstance(s, dict):
                _line(f"{name}: {label}", s, f"{s['GB/s']:>11.1f}")
        print(f"    (image: {rec['image_bytes']} bytes, {rec['values_used']} values used)")
    results["calls"] = calls = _child("calls", args)
    against = "the parent commit's library" if calls["parent_library"] else "this library"
    print(f"\n(b) the call against what a caller does today (wall, one process, ways alternating); 'before' is {against}'s")
    print(f"  the {args.size} x {args.size} map of 21 labels, strategy e, numiterations 5")
    print(head)
    for way, s in calls["label map"].items():
        if isinstance(s, dict):
            _line(way, s)
    _verdict(calls["label map"], "new - today")
    print(f"  {args.masks} masks of 64 x 64 at 1 bit through the batch, strategy e, numiterations 15")
    print(head)
    for way, s in calls["masks"].items():
        if isinstance(s, dict):
            _line(way, s)
    _verdict(calls["masks"], "new - today")
    results["existing"] = ex = _child("existing", args)
    against = "the parent commit's library" if ex["parent_library"] else "this library"
    print(f"\n(c) for information: zmx_png_optimize_device of a {args.size} x {args.size} RGBA8 image, \"auto\", numiterations 5; 'before' is {against}'s")
    print(head)
    for way in ("zmx_png_optimize_device, auto", "zmx_png_optimize_device, auto (before)"):
        _line(way, ex[way])
    _verdict(ex, "now - before")
    print()
    print(json.dumps({"repeat": args.repeat, "size": args.size, "masks": args.masks, "parent_lib": bool(args.parent_lib), "results": results}))


if __name__ == "__main__":
    main()
