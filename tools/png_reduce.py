"""Colour-type reduction of an image in device memory: what k_png_color_stats, k_png_color_key, k_png_convert,
zmx_png_optimize_device and its batch cost.

Three tables, each measured in a child process of its own; inside a process the ways that are compared alternate, after a
warm-up call of each, and a line gives the best of --repeat runs and the spread (max - min).
(a) the kernels alone, by HIP events (zmx_internal_png_color_ms), on 4096 x 4096 RGBA8 images: the statistics of a
    photograph-like image (more than 256 colours at once), of a 256-colour image (the full colour pass), of an opaque grey
    image and of an image with a key (k_png_color_key runs as well); the conversion to a palette of 8 bits, to grey of 1
    bit and to RGB; each beside one hipMemcpyAsync device to device of the image.  GB/s counts the algorithmic bytes: the
    image read once, the converted image written once (the copy: the image's bytes read and written).
(b) zmx_png_optimize_device of an image that cannot be reduced (noise RGBA with partial alpha), strategy e,
    numiterations 5, against zmx_png_encode_device of the same image — of the library at --parent-lib where one is given
    (the build of the commit before), else of this library; and for information both entries on the opaque photograph and
    on the 256-colour image, with the files' sizes.
(c) zmx_png_optimize_device_batch of 1 000 icons of 64 x 64 RGBA8 with at most 32 colours, numiterations 15, against
    zmx_png_encode_device_batch.

usage: python tools/png_reduce.py [--repeat 5] [--size 4096] [--icons 1000] [--parent-lib PATH]
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


def _images(w):
    """The 4096 x 4096 RGBA8 images of table (a), as numpy arrays."""
    import numpy as np
    rng = np.random.default_rng(11)
    photo = _image(w)
    colors = rng.integers(0, 256, size=(256, 4), dtype=np.uint8)
    colors[:, 3] = 255
    colors[:, 0] = np.arange(256)                       # (256 different ones for sure)
    smooth = ((np.add.outer(np.arange(w), np.arange(w)) // 16 + rng.integers(0, 3, size=(w, w))) % 256)
    pal256 = colors[smooth]
    g = ((np.add.outer(np.arange(w), np.arange(w)) // 8) % 256).astype(np.uint8)
    grey = np.stack([g, g, g, np.full_like(g, 255)], axis=-1)
    key = photo.copy()
    key[key[..., 0] == 7, 0] = 8
    key[100:200, 300:900] = (7, 7, 7, 0)
    mask = np.where(rng.integers(0, 40, size=(w, w)) == 0, 255, 0).astype(np.uint8)
    mask = np.stack([mask, mask, mask, np.full_like(mask, 255)], axis=-1)
    noise = photo.copy()
    noise[..., 3] = rng.integers(0, 256, size=(w, w), dtype=np.uint8)
    return {"photograph": photo, "256 colours": np.ascontiguousarray(pal256), "opaque grey": grey, "key": key, "mask": mask,
            "irreducible": noise}


def _kernels(args):
    import torch

    from batch_files import _Hip
    from zopfli_amd import Context, api
    lib = api.library()
    lib.zmx_internal_png_color_ms.argtypes = [ctypes.POINTER(ctypes.c_double)]
    lib.zmx_internal_png_color_ms.restype = None
    lib.zmx_set_kernel_timing(1)
    hip = _Hip()
    ctx = Context(0, lib)
    w = args.size
    nbytes = 4 * w * w
    imgs = _images(w)
    spare = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out_buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    ms3 = (ctypes.c_double * 3)()
    out = {"image_bytes": nbytes, "stats": {}, "convert": {}}
    for name in ("photograph", "256 colours", "opaque grey", "key"):
        d = torch.from_numpy(imgs[name]).cuda()
        torch.cuda.synchronize()
        runs = []
        for i in range(args.repeat + 1):
            st = ctx.png_color_stats_device(d)
            lib.zmx_internal_png_color_ms(ms3)
            copy = hip.copies_ms(spare.data_ptr(), [(d.data_ptr(), nbytes)])
            if i:
                runs.append((ms3[0], ms3[1], copy))
        rec = {"k_png_color_stats": _stats([r[0] for r in runs]), "one_hipMemcpyAsync": _stats([r[2] for r in runs])}
        rec["k_png_color_stats"]["GB/s"] = round(nbytes / 1e6 / rec["k_png_color_stats"]["best_ms"], 1)
        rec["one_hipMemcpyAsync"]["GB/s"] = round(2 * nbytes / 1e6 / rec["one_hipMemcpyAsync"]["best_ms"], 1)
        if any(r[1] for r in runs):
            rec["k_png_color_key"] = _stats([r[1] for r in runs])
            rec["k_png_color_key"]["GB/s"] = round(nbytes / 1e6 / rec["k_png_color_key"]["best_ms"], 1)
        rec["found"] = {"colored": st.colored, "key": st.key, "alpha": st.alpha, "numcolors": st.numcolors, "bits": st.bits}
        out["stats"][name] = rec
        del d
    for name, source in (("palette of 8 bits", "256 colours"), ("grey of 1 bit", "mask"), ("RGB of 8 bits", "photograph")):
        d = torch.from_numpy(imgs[source]).cuda()
        torch.cuda.synchronize()
        st = ctx.png_color_stats_device(d)
        mode = api.png_choose_color(st, w * w, lib=lib)
        bpp = (1 if mode.colortype == 3 else {0: 1, 2: 3, 4: 2, 6: 4}[mode.colortype]) * mode.bitdepth
        total = w * ((w * bpp + 7) // 8)
        runs = []
        for i in range(args.repeat + 1):
            ctx.png_convert_device(d, mode, out_buf)
            lib.zmx_internal_png_color_ms(ms3)
            copy = hip.copies_ms(spare.data_ptr(), [(d.data_ptr(), nbytes)])
            if i:
                runs.append((ms3[2], copy))
        rec = {"k_png_convert": _stats([r[0] for r in runs]), "one_hipMemcpyAsync": _stats([r[1] for r in runs])}
        rec["k_png_convert"]["GB/s"] = round((nbytes + total) / 1e6 / rec["k_png_convert"]["best_ms"], 1)
        rec["one_hipMemcpyAsync"]["GB/s"] = round(2 * nbytes / 1e6 / rec["one_hipMemcpyAsync"]["best_ms"], 1)
        rec["mode"] = {"colortype": mode.colortype, "bitdepth": mode.bitdepth, "palettesize": mode.palettesize, "output_bytes": total}
        out["convert"][name] = rec
        del d
    ctx.close()
    return out


def _whole(args):
    import torch

    from zopfli_amd import Context, ZopfliOptions, api
    lib = api.library()
    parent = api.library(args.parent_lib) if args.parent_lib else lib
    lib.zmx_internal_png_color_ms.argtypes = [ctypes.POINTER(ctypes.c_double)]
    lib.zmx_internal_png_color_ms.restype = None
    w = args.size
    imgs = _images(w)
    opt = ZopfliOptions(5)
    out = {"parent_library": bool(args.parent_lib)}
    for name in ("irreducible", "photograph", "256 colours"):
        d = torch.from_numpy(imgs[name]).cuda()
        torch.cuda.synchronize()
        sizes = {}

        def optimize():
            sizes["optimize"] = len(api.png_optimize_device(d, "e", opt, lib=lib))

        def encode():
            sizes["encode"] = len(api.png_encode_device(d, "e", opt, lib=parent))

        ms = _alternate({"zmx_png_optimize_device": optimize, "zmx_png_encode_device": encode}, args.repeat)
        rec = {k: _stats(v) for k, v in ms.items()}
        rec["bytes"] = sizes
        if name == "irreducible":
            # the entry's own added device time: the statistics, by HIP events
            lib.zmx_set_kernel_timing(1)
            ctx = Context(0, lib)
            ms3 = (ctypes.c_double * 3)()
            own = []
            for i in range(args.repeat + 1):
                ctx.png_color_stats_device(d)
                lib.zmx_internal_png_color_ms(ms3)
                if i:
                    own.append(ms3[0] + ms3[1])
            ctx.close()
            lib.zmx_set_kernel_timing(0)
            rec["statistics kernels (HIP events)"] = _stats(own)
            o, e = rec["zmx_png_optimize_device"], rec["zmx_png_encode_device"]
            rec["difference_ms"] = round(o["best_ms"] - e["best_ms"], 2)
            rec["allowed_ms"] = round(min(own) + o["spread_ms"] + e["spread_ms"], 2)
            rec["same_file"] = sizes["optimize"] == sizes["encode"]
        out[name] = rec
        del d
    return out


def _icons(args):
    import numpy as np
    import torch

    from zopfli_amd import ZopfliOptions, api
    lib = api.library()
    k, iw = args.icons, 64
    icons = []
    for i in range(k):
        rng = np.random.default_rng(500 + i)
        colors = rng.integers(0, 256, size=(int(rng.integers(2, 33)), 4), dtype=np.uint8)
        colors[:, 3] = 255
        y, x = np.mgrid[0:iw, 0:iw]
        idx = ((x // 4 + y // 6 + rng.integers(0, 2, size=(iw, iw))) % len(colors))
        icons.append(torch.from_numpy(np.ascontiguousarray(colors[idx])).cuda())
    torch.cuda.synchronize()
    opt = ZopfliOptions(15)
    got = {}

    def optimize():
        got["optimize"] = api.png_optimize_device_batch(icons, "e", opt, lib=lib)

    def encode():
        got["encode"] = api.png_encode_device_batch(icons, "e", opt, lib=lib)

    ms = _alternate({"zmx_png_optimize_device_batch": optimize, "zmx_png_encode_device_batch": encode}, args.repeat)
    out = {name: _stats(v) for name, v in ms.items()}
    kinds = {}
    for f in got["optimize"]:
        kinds[str(f[25])] = kinds.get(str(f[25]), 0) + 1
    out["bytes"] = {"optimize": sum(len(p) for p in got["optimize"]), "encode": sum(len(p) for p in got["encode"])}
    out["files_by_colour_type"] = kinds
    return out


TABLES = {"kernels": _kernels, "whole": _whole, "icons": _icons}


def _child(table, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", table, "--repeat", str(args.repeat), "--size", str(args.size),
           "--icons", str(args.icons)] + (["--parent-lib", args.parent_lib] if args.parent_lib else [])
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{table}: {r.stderr[-3000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def _line(name, s, extra=""):
    print(f"  {name:<52}{s['best_ms']:>12.3f}{s['spread_ms']:>11.3f}{extra}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--icons", type=int, default=1000)
    ap.add_argument("--parent-lib", default=None, help="libzopfli_amd.so of the commit before, for table (b)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(TABLES[args.child](args)), flush=True)
        return
    results = {}
    head = f"  {'':<52}{'best ms':>12}{'spread ms':>11}"
    results["kernels"] = ker = _child("kernels", args)
    print(f"(a) the kernels alone (HIP events) on {args.size} x {args.size} RGBA8, {ker['image_bytes']} bytes, best of {args.repeat} after a warm-up")
    print(head + "       GB/s")
    for name, rec in ker["stats"].items():
        for kernel in ("k_png_color_stats", "k_png_color_key", "one_hipMemcpyAsync"):
            if kernel in rec:
                _line(f"{name}: {kernel}", rec[kernel], f"{rec[kernel]['GB/s']:>11.1f}")
        print(f"    (found: {rec['found']})")
    for name, rec in ker["convert"].items():
        for kernel in ("k_png_convert", "one_hipMemcpyAsync"):
            _line(f"to {name}: {kernel}", rec[kernel], f"{rec[kernel]['GB/s']:>11.1f}")
        print(f"    (mode: {rec['mode']})")
    results["whole"] = whole = _child("whole", args)
    against = "the parent commit's library" if whole["parent_library"] else "this library"
    print(f"\n(b) {args.size} x {args.size} RGBA8, strategy e, numiterations 5 (wall, one process, ways alternating); "
          f"zmx_png_encode_device is {against}'s")
    print(head)
    for name in ("irreducible", "photograph", "256 colours"):
        rec = whole[name]
        for way in ("zmx_png_optimize_device", "zmx_png_encode_device", "statistics kernels (HIP events)"):
            if way in rec:
                _line(f"{name}: {way}", rec[way])
        print(f"    bytes {rec['bytes']}")
        if "difference_ms" in rec:
            print(f"    optimize - encode = {rec['difference_ms']} ms; allowed: the statistics + both spreads = {rec['allowed_ms']} ms: "
                  f"{'holds' if rec['difference_ms'] <= rec['allowed_ms'] else 'DOES NOT HOLD'};  same file size: {rec['same_file']}")
    results["icons"] = ico = _child("icons", args)
    print(f"\n(c) {args.icons} x 64 x 64 RGBA8 of at most 32 colours, strategy e, numiterations 15 (wall, one process, ways alternating)")
    print(head)
    for name, s in ico.items():
        if isinstance(s, dict) and "best_ms" in s:
            _line(name, s)
    print(f"    bytes {ico['bytes']};  the optimized files by colour type: {ico['files_by_colour_type']}")
    print()
    print(json.dumps({"repeat": args.repeat, "size": args.size, "icons": args.icons, "results": results}))


if __name__ == "__main__":
    main()
