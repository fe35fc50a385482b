"""zopflipng's --lossy_transparent on an image in device memory: what k_png_lossy_stats, k_png_lossy_carry and
k_png_lossy_fill cost, what the _lossy entries cost those who do not ask, and what the flag buys.

Four tables, each measured in a child process of its own; inside a process the ways that are compared alternate, after a
warm-up call of each, and a line gives the best of --repeat runs and the spread (max - min).
(a) the three kernels alone, by HIP events (zmx_internal_png_lossy_ms), on 4096 x 4096 RGBA8 images, out of place: fixed
    mode (a key stays possible); carry mode with short transparent runs; carry mode with every pixel transparent but the
    first 300, one of them with a partial alpha — every tile but the first passes its carry on, the worst case for the
    carry; no transparent pixel at all (the statistics alone).  Each beside one hipMemcpyAsync device to device of the
    image.  GB/s counts the algorithmic bytes: the image read once by the statistics, read and written once by the fill
    (and by the copy).
(b) zmx_png_optimize_device_lossy(lossy = 0) of an image that cannot be reduced (noise RGBA with partial alpha), strategy
    e, numiterations 5, against zmx_png_optimize_device of the library at --parent-lib where one is given (the build of
    the commit before), else of this library.  It may not be slower by more than the two spreads together.
(c) the same entry with _TRANSPARENT against lossy = 0 on an image the rewrite leaves as it is (the rewrite's own output
    fed back in), so that both ways deflate the same bytes.  Allowed: the kernels' own time by HIP events plus the two
    spreads.
(d) for information, what the flag buys: file sizes and times with and without it for a 4096 x 4096 sheet of sprites with
    garbage under alpha 0, and for --icons icons of 64 x 64 through the batch (numiterations 15).

usage: python tools/png_lossy.py [--repeat 5] [--size 4096] [--icons 1000] [--parent-lib PATH]
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


def _irreducible(w):
    import numpy as np
    img = _image(w)
    img[..., 3] = np.random.default_rng(11).integers(1, 256, size=(w, w), dtype=np.uint8)
    return img


def _images(w):
    """The RGBA8 images of table (a), as numpy arrays."""
    import numpy as np
    rng = np.random.default_rng(23)
    garbage = rng.integers(0, 256, size=(w, w, 3), dtype=np.uint8)
    fixed = _image(w)
    hole = np.zeros((w, w), dtype=bool)
    hole[w // 8:w // 2, w // 4:3 * w // 4] = True
    hole |= rng.integers(0, 50, size=(w, w)) == 0
    fixed[hole, :3] = garbage[hole]
    fixed[hole, 3] = 0
    short = _irreducible(w)
    runs = (rng.integers(0, 12, size=(w, w // 8)) == 0).repeat(8, axis=1)
    short[runs, :3] = garbage[runs]
    short[runs, 3] = 0
    worst = np.concatenate([garbage, np.zeros((w, w, 1), dtype=np.uint8)], axis=2)
    worst[0, :300, 3] = 255
    worst[0, :300, 0] = np.arange(300) % 256
    worst[0, :300, 1] = np.arange(300) // 256
    worst[0, 7, 3] = 128
    return {"fixed (key)": fixed, "carry, short runs": short, "carry, all transparent but 300": np.ascontiguousarray(worst),
            "no transparent pixel": _irreducible(w)}


def _sprites(w):
    """A sheet of 64 x 64 sprites: shaded discs with a soft edge, whatever the renderer had left under alpha 0."""
    import numpy as np
    rng = np.random.default_rng(31)
    y, x = np.mgrid[0:w, 0:w]
    cy, cx = y % 64 - 31.5, x % 64 - 31.5
    r = np.sqrt(cy * cy + cx * cx)
    cell = (y // 64) * (w // 64) + x // 64
    base = rng.integers(0, 256, size=(cell.max() + 1, 3))
    img = np.empty((w, w, 4), dtype=np.uint8)
    shade = np.clip(1.0 - r / 40.0, 0, 1)
    for k in range(3):
        img[..., k] = np.clip(base[cell, k] * shade + rng.integers(0, 3, size=(w, w)), 0, 255)
    alpha = np.clip((26.0 - r) * 64.0, 0, 255)
    img[..., 3] = alpha
    clear = img[..., 3] == 0
    img[clear, :3] = rng.integers(0, 256, size=(int(clear.sum()), 3), dtype=np.uint8)
    return img


def _icons(k, iw=64):
    import numpy as np
    out = []
    for i in range(k):
        rng = np.random.default_rng(900 + i)
        colors = rng.integers(0, 256, size=(int(rng.integers(2, 33)), 4), dtype=np.uint8)
        colors[:, 3] = 255
        y, x = np.mgrid[0:iw, 0:iw]
        img = colors[(x // 4 + y // 6 + rng.integers(0, 2, size=(iw, iw))) % len(colors)]
        clear = (x - 31.5) ** 2 + (y - 31.5) ** 2 > 28 ** 2
        img[clear, :3] = rng.integers(0, 256, size=(int(clear.sum()), 3), dtype=np.uint8)
        img[clear, 3] = 0
        out.append(np.ascontiguousarray(img))
    return out


def _bind_ms(lib):
    lib.zmx_internal_png_lossy_ms.argtypes = [ctypes.POINTER(ctypes.c_double)]
    lib.zmx_internal_png_lossy_ms.restype = None


def _kernels(args):
    import torch

    from batch_files import _Hip
    from zopfli_amd import Context, api
    lib = api.library()
    _bind_ms(lib)
    lib.zmx_set_kernel_timing(1)
    hip = _Hip()
    ctx = Context(0, lib)
    w = args.size
    nbytes = 4 * w * w
    out_buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    spare = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    ms3 = (ctypes.c_double * 3)()
    out = {"image_bytes": nbytes, "images": {}}
    for name, img in _images(w).items():
        d = torch.from_numpy(img).cuda()
        torch.cuda.synchronize()
        runs = []
        for i in range(args.repeat + 1):
            info = ctx.png_lossy_transparent_device(d, out_buf)
            lib.zmx_internal_png_lossy_ms(ms3)
            copy = hip.copies_ms(spare.data_ptr(), [(d.data_ptr(), nbytes)])
            if i:
                runs.append((ms3[0], ms3[1], ms3[2], copy))
        rec = {"k_png_lossy_stats": _stats([r[0] for r in runs]), "one_hipMemcpyAsync": _stats([r[3] for r in runs])}
        rec["k_png_lossy_stats"]["GB/s"] = round(nbytes / 1e6 / rec["k_png_lossy_stats"]["best_ms"], 1)
        rec["one_hipMemcpyAsync"]["GB/s"] = round(2 * nbytes / 1e6 / rec["one_hipMemcpyAsync"]["best_ms"], 1)
        if info.mode == 2:
            rec["k_png_lossy_carry"] = _stats([r[1] for r in runs])
        if info.mode != 0:
            rec["k_png_lossy_fill"] = _stats([r[2] for r in runs])
            rec["k_png_lossy_fill"]["GB/s"] = round(2 * nbytes / 1e6 / rec["k_png_lossy_fill"]["best_ms"], 1)
        rec["all three"] = _stats([r[0] + r[1] + r[2] for r in runs])
        rec["found"] = {"mode": info.mode, "partial_alpha": info.partial_alpha, "numcolors": info.numcolors,
                        "first_transparent": None if info.first_transparent == 2 ** 64 - 1 else info.first_transparent}
        out["images"][name] = rec
        del d
    ctx.close()
    return out


def _unasked(args):
    import torch

    from zopfli_amd import ZopfliOptions, api
    lib = api.library()
    parent = api.library(args.parent_lib) if args.parent_lib else lib
    d = torch.from_numpy(_irreducible(args.size)).cuda()
    torch.cuda.synchronize()
    opt = ZopfliOptions(5)
    fn = lib.zmx_png_optimize_device_lossy
    fn.argtypes = [ctypes.POINTER(ZopfliOptions), ctypes.POINTER(api.PngImage), ctypes.c_int, ctypes.c_char_p, ctypes.c_uint,
                   ctypes.POINTER(api._u8p), ctypes.POINTER(ctypes.c_size_t)]
    fn.restype = ctypes.c_int
    sizes = {}

    def lossy0():
        out, size = api._u8p(), ctypes.c_size_t(0)
        im = api._png_image(d)
        assert fn(ctypes.byref(opt), ctypes.byref(im), 6, None, 0, ctypes.byref(out), ctypes.byref(size)) == 0
        sizes["lossy0"] = len(api._take(out, size))

    def before():
        sizes["parent"] = len(api.png_optimize_device(d, "e", opt, lib=parent))

    ms = _alternate({"zmx_png_optimize_device_lossy(lossy = 0)": lossy0, "zmx_png_optimize_device (before)": before}, args.repeat)
    rec = {k: _stats(v) for k, v in ms.items()}
    a, b = rec["zmx_png_optimize_device_lossy(lossy = 0)"], rec["zmx_png_optimize_device (before)"]
    rec["difference_ms"] = round(a["best_ms"] - b["best_ms"], 2)
    rec["allowed_ms"] = round(a["spread_ms"] + b["spread_ms"], 2)
    rec["bytes"] = sizes
    rec["parent_library"] = bool(args.parent_lib)
    return rec


def _asked(args):
    import torch

    from zopfli_amd import Context, ZopfliOptions, api
    lib = api.library()
    _bind_ms(lib)
    w = args.size
    d = torch.from_numpy(_images(w)["carry, short runs"]).cuda()
    torch.cuda.synchronize()
    ctx = Context(0, lib)
    # (the rewrite's own output: the rewrite leaves it as it is)
    info = ctx.png_lossy_transparent_device(d, d)
    before = d.clone()
    assert ctx.png_lossy_transparent_device(d, d).mode == info.mode and bool(torch.equal(d, before))
    opt = ZopfliOptions(5)
    sizes = {}

    def asked():
        sizes["with"] = len(api.png_optimize_device(d, "e", opt, lib=lib, lossy_transparent=True))

    def unasked():
        sizes["without"] = len(api.png_optimize_device(d, "e", opt, lib=lib))

    ms = _alternate({"with _TRANSPARENT": asked, "lossy = 0": unasked}, args.repeat)
    rec = {k: _stats(v) for k, v in ms.items()}
    lib.zmx_set_kernel_timing(1)
    spare = torch.empty_like(d)
    ms3 = (ctypes.c_double * 3)()
    own = []
    for i in range(args.repeat + 1):
        ctx.png_lossy_transparent_device(d, spare)
        lib.zmx_internal_png_lossy_ms(ms3)
        if i:
            own.append(ms3[0] + ms3[1] + ms3[2])
    lib.zmx_set_kernel_timing(0)
    ctx.close()
    rec["the three kernels (HIP events)"] = _stats(own)
    a, b = rec["with _TRANSPARENT"], rec["lossy = 0"]
    rec["difference_ms"] = round(a["best_ms"] - b["best_ms"], 2)
    rec["allowed_ms"] = round(min(own) + a["spread_ms"] + b["spread_ms"], 2)
    rec["bytes"] = sizes
    rec["mode"] = info.mode
    return rec


def _payoff(args):
    import torch

    from zopfli_amd import ZopfliOptions, api
    lib = api.library()
    out = {}
    d = torch.from_numpy(_sprites(args.size)).cuda()
    torch.cuda.synchronize()
    sizes = {}
    for label, opt in (("sprites", ZopfliOptions(5)),):
        def with_flag():
            sizes["with"] = len(api.png_optimize_device(d, "e", opt, lib=lib, lossy_transparent=True))

        def without():
            sizes["without"] = len(api.png_optimize_device(d, "e", opt, lib=lib))

        ms = _alternate({"with _TRANSPARENT": with_flag, "lossy = 0": without}, args.repeat)
        out[label] = {k: _stats(v) for k, v in ms.items()}
        out[label]["bytes"] = dict(sizes)
    del d
    icons = [torch.from_numpy(i).cuda() for i in _icons(args.icons)]
    torch.cuda.synchronize()
    opt = ZopfliOptions(15)
    got = {}

    def batch_with():
        got["with"] = api.png_optimize_device_batch(icons, "e", opt, lib=lib, lossy_transparent=True)

    def batch_without():
        got["without"] = api.png_optimize_device_batch(icons, "e", opt, lib=lib)

    ms = _alternate({"with _TRANSPARENT": batch_with, "lossy = 0": batch_without}, args.repeat)
    out["icons"] = {k: _stats(v) for k, v in ms.items()}
    out["icons"]["bytes"] = {k: sum(len(p) for p in v) for k, v in got.items()}
    kinds = {}
    for k, files in got.items():
        kinds[k] = {}
        for f in files:
            kinds[k][str(f[25])] = kinds[k].get(str(f[25]), 0) + 1
    out["icons"]["files_by_colour_type"] = kinds
    return out


TABLES = {"kernels": _kernels, "unasked": _unasked, "asked": _asked, "payoff": _payoff}


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
    ap.add_argument("--parent-lib", default=None, help="libzopfli_amd.so of the commit before, for table (b)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(TABLES[args.child](args)), flush=True)
        return
    results = {}
    head = f"  {'':<60}{'best ms':>12}{'spread ms':>11}"
    results["kernels"] = ker = _child("kernels", args)
    print(f"(a) the kernels alone (HIP events) on {args.size} x {args.size} RGBA8, {ker['image_bytes']} bytes, out of place, "
          f"best of {args.repeat} after a warm-up")
    print(head + "       GB/s")
    for name, rec in ker["images"].items():
        for kernel in ("k_png_lossy_stats", "k_png_lossy_carry", "k_png_lossy_fill", "all three", "one_hipMemcpyAsync"):
            if kernel in rec:
                _line(f"{name}: {kernel}", rec[kernel], f"{rec[kernel]['GB/s']:>11.1f}" if "GB/s" in rec[kernel] else "")
        print(f"    (found: {rec['found']})")
    results["unasked"] = un = _child("unasked", args)
    against = "the parent commit's library" if un["parent_library"] else "this library"
    print(f"\n(b) {args.size} x {args.size} RGBA8 that cannot be reduced, strategy e, numiterations 5 (wall, one process, ways alternating); "
          f"'before' is {against}'s")
    print(head)
    for way in ("zmx_png_optimize_device_lossy(lossy = 0)", "zmx_png_optimize_device (before)"):
        _line(way, un[way])
    print(f"    bytes {un['bytes']}")
    print(f"    lossy = 0 - before = {un['difference_ms']} ms; allowed: both spreads = {un['allowed_ms']} ms: "
          f"{'holds' if un['difference_ms'] <= un['allowed_ms'] else 'DOES NOT HOLD'}")
    results["asked"] = asked = _child("asked", args)
    print(f"\n(c) zmx_png_optimize_device_lossy on a {args.size} x {args.size} RGBA8 image the rewrite leaves as it is (mode {asked['mode']}), "
          f"strategy e, numiterations 5")
    print(head)
    for way in ("with _TRANSPARENT", "lossy = 0", "the three kernels (HIP events)"):
        _line(way, asked[way])
    print(f"    bytes {asked['bytes']}")
    print(f"    with - without = {asked['difference_ms']} ms; allowed: the kernels + both spreads = {asked['allowed_ms']} ms: "
          f"{'holds' if asked['difference_ms'] <= asked['allowed_ms'] else 'DOES NOT HOLD'}")
    results["payoff"] = pay = _child("payoff", args)
    print(f"\n(d) what the flag buys (wall, one process, ways alternating): a {args.size} x {args.size} sheet of sprites, numiterations 5; "
          f"{args.icons} icons of 64 x 64 through zmx_png_optimize_device_batch_lossy, numiterations 15")
    print(head)
    for label in ("sprites", "icons"):
        for way in ("with _TRANSPARENT", "lossy = 0"):
            _line(f"{label}: {way}", pay[label][way])
        print(f"    bytes {pay[label]['bytes']}" + (f";  files by colour type: {pay[label]['files_by_colour_type']}" if label == "icons" else ""))
    print()
    print(json.dumps({"repeat": args.repeat, "size": args.size, "icons": args.icons, "results": results}))


if __name__ == "__main__":
    main()
