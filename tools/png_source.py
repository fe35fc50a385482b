"""Strided, planar, float and 16-bit sources of the device PNG entries: what k_png_pack costs beside a plain copy and beside
the torch chain a caller writes today, what png_encode_device(PngSource) saves that caller, and that the existing path is
as fast as it was.

Three tables, each measured in a child process of its own on one device; inside a process the ways that are compared
alternate, after a warm-up of each, and a line gives the best of --repeat runs and the spread (max - min).
(a) k_png_pack alone, by HIP events (zmx_internal_png_pack_ms), against one hipMemcpyAsync device to device of the packed
    image's bytes and against the torch chain (events on torch's stream):
      SIZE x SIZE RGBA8 from (4, H, W) float32         (x.clamp(0, 1) * 255 + 0.5).to(uint8).permute(1, 2, 0).contiguous()
      SIZE x SIZE RGBA8 from (H, W, 4) uint8, pitched  frame[:, :W].contiguous()
      SIZE x SIZE RGB16 from (3, H, W) uint16          permute, contiguous, the bytes of every sample swapped through a uint8 view
      ICONS x 64 x 64 RGBA8 out of one NCHW float32    ONE launch against ICONS torch chains
    GB/s counts the algorithmic bytes: the samples read once and the packed image written once (the copy: read and written).
    A case whose algorithmic bytes are below 256 MB lies inside the Infinity Cache; the table says which.
(b) the calls (wall): png_encode_device[_batch](PngSource) of this library against the torch chain plus png_encode_device
    [_batch] of the library at --parent-lib (the build of the commit before; else this library): the SIZE x SIZE RGBA8
    image from CHW float32 at numiterations 5, the icons through the batch at numiterations 15, strategy e.  The files must
    be equal, and the new entry may not be slower than what the caller does today by more than the two spreads together.
(c) for information: png_encode_device of a plain SIZE x SIZE RGBA8 image, strategy e, this library against the parent's.

usage: python tools/png_source.py [--repeat 5] [--size 4096] [--icons 1000] [--parent-lib PATH]
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

CACHE_MB = 256   # the Infinity Cache of one MI355X


def _parent(args, lib):
    from zopfli_amd import api
    if not args.parent_lib:
        return lib
    parent = api.bind(ctypes.CDLL(os.path.abspath(args.parent_lib)))
    parent.zmx_set_kernel_timing(0)
    return parent


def _icons(k, iw=64):
    """(k, 4, iw, iw) float32 in [0, 1]: small gradients with noise, each another."""
    import numpy as np
    rng = np.random.default_rng(11)
    y, x = np.mgrid[0:iw, 0:iw]
    out = np.empty((k, 4, iw, iw), dtype=np.float32)
    for i in range(k):
        a, b = rng.integers(1, 5, size=2)
        img = np.stack([(a * x + i) % 256, (b * y + 2 * i) % 256, ((x + y) * a // 2) % 256, np.full_like(x, 255)]).astype(np.int32)
        img[:3] += rng.integers(-2, 3, size=(3, iw, iw))
        out[i] = np.clip(img, 0, 255).astype(np.float32) / 255.0
    return out


def _chain(x):
    import torch
    return (x.clamp(0, 1) * 255 + 0.5).to(torch.uint8).permute(1, 2, 0).contiguous()


def _torch_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    keep = fn()
    b.record()
    b.synchronize()
    del keep
    return a.elapsed_time(b)


def _kernels(args):
    import numpy as np
    import torch

    from batch_files import _Hip
    from zopfli_amd import Context, api
    lib = api.library()
    lib.zmx_internal_png_pack_ms.restype = ctypes.c_double
    lib.zmx_set_kernel_timing(1)
    hip = _Hip()
    ctx = Context(0, lib)
    w = args.size
    rgba = _image(w)
    chw = torch.from_numpy(np.ascontiguousarray(rgba.transpose(2, 0, 1)).astype(np.float32) / 255.0).cuda()
    pitch = w + 64
    frame = torch.zeros((w, pitch, 4), dtype=torch.uint8, device="cuda")
    frame[:, :w] = torch.from_numpy(rgba).cuda()
    rgb16 = torch.from_numpy((rgba[:, :, :3].astype(np.uint16) * 257).transpose(2, 0, 1).copy()).cuda()
    icons = torch.from_numpy(_icons(args.icons)).cuda()
    out_buf = torch.empty(6 * w * w, dtype=torch.uint8, device="cuda")
    spare = torch.empty(6 * w * w, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def swap16():
        v = rgb16.permute(1, 2, 0).contiguous().view(torch.uint8).reshape(w, w, 3, 2)
        return v.flip(-1).contiguous()

    cases = [
        (f"{w} x {w} RGBA8 from CHW float32", [api.PngSource(chw, "CHW")], 16 * w * w, 4 * w * w, lambda: _chain(chw), 1),
        (f"{w} x {w} RGBA8 from HWC uint8, pitched", [api.PngSource(frame[:, :w], "HWC")], 4 * w * w, 4 * w * w, lambda: frame[:, :w].contiguous(), 1),
        (f"{w} x {w} RGB16 from CHW uint16", [api.PngSource(rgb16, "CHW")], 6 * w * w, 6 * w * w, swap16, 1),
        (f"{args.icons} x 64 x 64 RGBA8 out of one NCHW float32", api.png_sources(icons), 16 * 4096 * args.icons, 4 * 4096 * args.icons,
         lambda: [_chain(x) for x in icons], args.icons),
    ]
    out = {}
    for name, sources, read, written, chain, launches in cases:
        each = written // len(sources)
        outs = [(out_buf.data_ptr() + k * each, each) for k in range(len(sources))]
        runs = []
        for i in range(args.repeat + 1):
            ctx.png_pack_device(sources, outs)
            pack = lib.zmx_internal_png_pack_ms()
            copy = hip.copies_ms(spare.data_ptr(), [(out_buf.data_ptr(), written)])
            torch_ms = _torch_ms(chain)
            if i:
                runs.append((pack, copy, torch_ms))
        rec = {"read": read, "written": written, "inside_cache": (read + written) / 1e6 < CACHE_MB}
        for k, (label, moved) in enumerate(((f"k_png_pack, one launch", read + written), ("one hipMemcpyAsync of the packed bytes", 2 * written),
                                            (f"the torch chain ({launches} of them)" if launches > 1 else "the torch chain", read + written))):
            rec[label] = _stats([r[k] for r in runs])
            rec[label]["GB/s"] = round(moved / 1e6 / rec[label]["best_ms"], 1)
        out[name] = rec
    ctx.close()
    return out


def _calls(args):
    import numpy as np
    import torch

    from zopfli_amd import ZopfliOptions, api
    lib = api.library()
    lib.zmx_set_kernel_timing(0)
    parent = _parent(args, lib)
    w = args.size
    out = {"parent_library": bool(args.parent_lib)}
    chw = torch.from_numpy(np.ascontiguousarray(_image(w).transpose(2, 0, 1)).astype(np.float32) / 255.0).cuda()
    torch.cuda.synchronize()
    opt = ZopfliOptions(5)
    got = {}

    def today():
        got["today"] = api.png_encode_device(_chain(chw), "e", opt, lib=parent)

    def new():
        got["new"] = api.png_encode_device(api.PngSource(chw, "CHW"), "e", opt, lib=lib)

    ms = _alternate({"png_encode_device(PngSource)": new, "torch chain + png_encode_device (before)": today}, args.repeat)
    rec = {k: _stats(v) for k, v in ms.items()}
    rec["files_equal"] = got["new"] == got["today"]
    rec["bytes"] = len(got["new"])
    out["image"] = rec
    del chw
    icons = torch.from_numpy(_icons(args.icons)).cuda()
    torch.cuda.synchronize()
    opt15 = ZopfliOptions(15)

    def batch_today():
        got["today"] = api.png_encode_device_batch([_chain(x) for x in icons], "e", opt15, lib=parent)

    def batch_new():
        got["new"] = api.png_encode_device_batch(api.png_sources(icons), "e", opt15, lib=lib)

    ms = _alternate({"png_encode_device_batch(png_sources)": batch_new, "torch chains + png_encode_device_batch (before)": batch_today}, args.repeat)
    rec = {k: _stats(v) for k, v in ms.items()}
    rec["files_equal"] = got["new"] == got["today"]
    rec["bytes"] = sum(len(f) for f in got["new"])
    out["icons"] = rec
    for rec in (out["image"], out["icons"]):
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
        got["now"] = api.png_encode_device(d, "e", opt, lib=lib)

    def before():
        got["before"] = api.png_encode_device(d, "e", opt, lib=parent)

    ms = _alternate({"png_encode_device, e": now, "png_encode_device, e (before)": before}, args.repeat)
    rec = {k: _stats(v) for k, v in ms.items()}
    a, b = rec["png_encode_device, e"], rec["png_encode_device, e (before)"]
    rec["difference_ms"] = round(a["best_ms"] - b["best_ms"], 2)
    rec["allowed_ms"] = round(a["spread_ms"] + b["spread_ms"], 2)
    rec["files_equal"] = got["now"] == got["before"]
    rec["bytes"] = len(got["now"])
    rec["parent_library"] = bool(args.parent_lib)
    return rec


TABLES = {"kernels": _kernels, "calls": _calls, "existing": _existing}


def _child(table, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", table, "--repeat", str(args.repeat), "--size", str(args.size),
           "--icons", str(args.icons)] + (["--parent-lib", args.parent_lib] if args.parent_lib else [])
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
    ap.add_argument("--icons", type=int, default=1000)
    ap.add_argument("--parent-lib", default=None, help="libzopfli_amd.so of the commit before, for tables (b) and (c)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(TABLES[args.child](args)), flush=True)
        return
    results = {}
    head = f"  {'':<72}{'best ms':>12}{'spread ms':>11}"
    results["kernels"] = ker = _child("kernels", args)
    print(f"(a) k_png_pack alone (HIP events), best of {args.repeat} after a warm-up")
    print(head + "       GB/s")
    for name, rec in ker.items():
        for label, s in rec.items():
            if isinstance(s, dict):
                _line(f"{name}: {label}", s, f"{s['GB/s']:>11.1f}")
        print(f"    ({rec['read']} bytes read, {rec['written']} written: {'inside' if rec['inside_cache'] else 'larger than'} the {CACHE_MB} MB Infinity Cache)")
    results["calls"] = calls = _child("calls", args)
    against = "the parent commit's library" if calls["parent_library"] else "this library"
    print(f"\n(b) the call against what a caller does today (wall, one process, ways alternating); 'before' is {against}'s")
    print(f"  the {args.size} x {args.size} RGBA8 image from CHW float32, strategy e, numiterations 5")
    print(head)
    for way, s in calls["image"].items():
        if isinstance(s, dict):
            _line(way, s)
    _verdict(calls["image"], "new - today")
    print(f"  {args.icons} icons of 64 x 64 out of one NCHW float32 tensor through the batch, strategy e, numiterations 15")
    print(head)
    for way, s in calls["icons"].items():
        if isinstance(s, dict):
            _line(way, s)
    _verdict(calls["icons"], "new - today")
    results["existing"] = ex = _child("existing", args)
    against = "the parent commit's library" if ex["parent_library"] else "this library"
    print(f"\n(c) for information: png_encode_device of a plain {args.size} x {args.size} RGBA8 image, strategy e, numiterations 5; 'before' is {against}'s")
    print(head)
    for way in ("png_encode_device, e", "png_encode_device, e (before)"):
        _line(way, ex[way])
    _verdict(ex, "now - before")
    print()
    print(json.dumps({"repeat": args.repeat, "size": args.size, "icons": args.icons, "parent_lib": bool(args.parent_lib), "results": results}))


if __name__ == "__main__":
    main()
