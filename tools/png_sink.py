"""Decoding into strided, planar, float and 16-bit sinks: what k_png_unpack costs beside a plain copy and beside the torch
chain a caller runs today on the decoder's output, what png_decode_tensors saves that caller, and that the existing decode
entry is as fast as it was.

Three tables, each measured in a child process of its own on one device; inside a process the ways that are compared
alternate, after a warm-up of each, and a line gives the best of --repeat runs and the spread (max - min).
(a) k_png_unpack alone, by HIP events (zmx_internal_png_unpack_ms), against one hipMemcpyAsync device to device of as many
    bytes as the sink holds and against the torch chain (events on torch's stream):
      SIZE x SIZE RGBA8 to CHW float32 RGB             t[..., :3].permute(2, 0, 1).float().div(255)
      SIZE x SIZE RGBA8 to a pitched HWC uint8 BGRA    frame[:, :W].copy_(t[..., [2, 1, 0, 3]])
      SIZE x SIZE RGB16 to CHW uint16                  the own-mode bytes of every sample swapped through a uint8 view, permute, contiguous
      ICONS x 64 x 64 RGBA8 into one NCHW float32      ONE launch against ICONS torch chains
    GB/s counts the algorithmic bytes: the pixels read once and the samples written once (the copy: read and written).
    A case whose algorithmic bytes are below 256 MB lies inside the Infinity Cache; the table says which.
(b) the calls (wall): png_decode_tensors of this library against png_decode_device_batch(rgba8) of the library at
    --parent-lib (the build of the commit before; else this library) plus the torch chain per image and a stack: ICONS icon
    files of 64 x 64, RGBA8 and 16-colour palette files.  The tensors are compared: torch divides by a scalar on the
    device by multiplying with the fp32 reciprocal, the sink divides, so float32 values may differ by one unit in the last
    place (the table counts them) and must equal the chain computed on the host.
(c) png_decode_device_batch(rgba8) of the same files, this library against the parent's, in one process: the existing entry
    may not be slower than the parent's by more than the two spreads together.

usage: python tools/png_sink.py [--repeat 5] [--size 4096] [--icons 1000] [--parent-lib PATH]
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

from png_decode import _icons  # noqa: E402
from png_device import _alternate, _image, _stats  # noqa: E402
from png_source import CACHE_MB, _parent, _torch_ms  # noqa: E402


def _mode(api, w, h, colortype, bitdepth):
    r = api.PngDecodeResult()
    r.width, r.height, r.colortype, r.bitdepth = w, h, colortype, bitdepth
    r.outsize = r.outsize_own = w * h * {2: 3, 6: 4}[colortype] * bitdepth // 8
    r.outsize_rgba8 = 4 * w * h
    return r


def _kernels(args):
    import numpy as np
    import torch

    from batch_files import _Hip
    from zopfli_amd import Context, api
    lib = api.library()
    lib.zmx_internal_png_unpack_ms.restype = ctypes.c_double
    lib.zmx_set_kernel_timing(1)
    hip = _Hip()
    ctx = Context(0, lib)
    w, n = args.size, args.icons
    rgba = torch.from_numpy(_image(w)).cuda()
    rgb16 = torch.from_numpy(np.ascontiguousarray((_image(w)[:, :, :3].astype(np.uint16) * 257 + 1).astype(">u2")).view(np.uint8).reshape(w, w, 6)).cuda()
    icons = torch.from_numpy(np.stack(_icons(np, n, 0))).cuda()
    chw = torch.empty((3, w, w), dtype=torch.float32, device="cuda")
    frame = torch.zeros((w, w + 64, 4), dtype=torch.uint8, device="cuda")
    chw16 = torch.empty((3, w, w), dtype=torch.uint16, device="cuda")
    batch = torch.empty((n, 3, 64, 64), dtype=torch.float32, device="cuda")
    spare = torch.empty(12 * w * w, dtype=torch.uint8, device="cuda")
    spare2 = torch.empty(12 * w * w, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def bgra():
        frame[:, :w].copy_(rgba[..., [2, 1, 0, 3]])

    def swap16():
        return rgb16.view(w, w, 3, 2).flip(-1).contiguous().view(torch.uint16).reshape(w, w, 3).permute(2, 0, 1).contiguous()

    def icon_chains():
        for i in range(n):
            batch[i] = icons[i][..., :3].permute(2, 0, 1).float().div(255)

    cases = [
        (f"{w} x {w} RGBA8 to CHW float32 RGB", [_mode(api, w, w, 6, 8)], [rgba], [api.PngSink(chw, "CHW")], 4 * w * w, 12 * w * w,
         lambda: rgba[..., :3].permute(2, 0, 1).float().div(255), 1),
        (f"{w} x {w} RGBA8 to a pitched HWC uint8 BGRA frame", [_mode(api, w, w, 6, 8)], [rgba], [api.PngSink(frame[:, :w], "HWC", "BGRA")], 4 * w * w,
         4 * w * w, bgra, 1),
        (f"{w} x {w} RGB16 to CHW uint16", [_mode(api, w, w, 2, 16)], [rgb16], [api.PngSink(chw16, "CHW")], 6 * w * w, 6 * w * w, swap16, 1),
        (f"{n} x 64 x 64 RGBA8 into one NCHW float32", [_mode(api, 64, 64, 6, 8)] * n, [icons[i] for i in range(n)], api.png_sinks(batch), 4 * 4096 * n,
         12 * 4096 * n, icon_chains, n),
    ]
    out = {}
    for name, modes, owns, sinks, read, written, chain, launches in cases:
        runs = []
        for i in range(args.repeat + 1):
            ctx.png_unpack_device(modes, owns, sinks)
            unpack = lib.zmx_internal_png_unpack_ms()
            copy = hip.copies_ms(spare.data_ptr(), [(spare2.data_ptr(), written)])
            torch_ms = _torch_ms(chain)
            if i:
                runs.append((unpack, copy, torch_ms))
        rec = {"read": read, "written": written, "inside_cache": (read + written) / 1e6 < CACHE_MB}
        for k, (label, moved) in enumerate((("k_png_unpack, one launch", read + written), ("one hipMemcpyAsync of the sink's bytes", 2 * written),
                                            (f"the torch chain ({launches} of them)" if launches > 1 else "the torch chain", read + written))):
            rec[label] = _stats([r[k] for r in runs])
            rec[label]["GB/s"] = round(moved / 1e6 / rec[label]["best_ms"], 1)
        out[name] = rec
    # (what was stored is what the chain gives where torch's div is a division: on the host)
    ctx.png_unpack_device(cases[0][1], cases[0][2], cases[0][3])
    out["equal"] = bool(torch.equal(chw.cpu(), rgba.cpu()[..., :3].permute(2, 0, 1).float().div(255)))
    ctx.close()
    return out


def _icon_files(api, lib, np, torch, count, colours):
    from zopfli_amd import ZopfliOptions
    if colours:
        imgs = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in _icons(np, count, colours)]
        return api.png_optimize_device_batch(imgs, "e", ZopfliOptions(2), lib=lib)
    imgs = [torch.from_numpy(a).cuda() for a in _icons(np, count, 0)]
    return api.png_encode_device_batch(imgs, "e", ZopfliOptions(2), lib=lib)


def _resident(torch, made):
    blob, offsets = bytearray(), []
    for f in made:
        blob += bytes(-len(blob) % 16)
        offsets.append(len(blob))
        blob += bytes(f)
    arena = torch.frombuffer(blob, dtype=torch.uint8).cuda()
    return arena, [(arena.data_ptr() + o, len(f)) for o, f in zip(offsets, made)]


def _calls(args):
    import numpy as np
    import torch

    from zopfli_amd import api
    lib = api.library()
    lib.zmx_set_kernel_timing(0)
    parent = _parent(args, lib)
    out = {"parent_library": bool(args.parent_lib)}
    for name, colours in (("RGBA8", 0), ("16-colour palette", 16)):
        arena, files = _resident(torch, _icon_files(api, lib, np, torch, args.icons, colours))
        torch.cuda.synchronize()
        got = {}

        def today():
            _, made = api.png_decode_device_batch(files, "rgba8", lib=parent)
            got["today"] = torch.stack([t[..., :3].permute(2, 0, 1).float().div(255) for t in made])
            torch.cuda.synchronize()

        def new():
            got["new"] = api.png_decode_tensors(files, lib=lib)[1]
            torch.cuda.synchronize()

        def existing_now():
            got["now"] = api.png_decode_device_batch(files, "rgba8", lib=lib)[1]

        def existing_before():
            got["before"] = api.png_decode_device_batch(files, "rgba8", lib=parent)[1]

        ms = _alternate({"png_decode_tensors": new, "png_decode_device_batch(rgba8) + torch chains (before)": today}, args.repeat)
        rec = {k: _stats(v) for k, v in ms.items()}
        rec["tensors_equal"] = bool(torch.equal(got["new"], got["today"]))
        # (torch's div by a scalar on the device multiplies by the fp32 reciprocal; the sink divides)
        rec["values_differing"] = int((got["new"] != got["today"]).sum())
        rec["max_abs_difference"] = float((got["new"] - got["today"]).abs().max())
        rec["equal_to_the_chain_on_the_host"] = bool(torch.equal(got["new"].cpu(), torch.stack(
            [t.cpu()[..., :3].permute(2, 0, 1).float().div(255) for t in api.png_decode_device_batch(files, "rgba8", lib=parent)[1]])))
        a, b = rec["png_decode_tensors"], rec["png_decode_device_batch(rgba8) + torch chains (before)"]
        rec["difference_ms"] = round(a["best_ms"] - b["best_ms"], 2)
        rec["allowed_ms"] = round(a["spread_ms"] + b["spread_ms"], 2)
        out[name] = rec
        ms = _alternate({"png_decode_device_batch(rgba8)": existing_now, "png_decode_device_batch(rgba8) (before)": existing_before}, args.repeat)
        rec = {k: _stats(v) for k, v in ms.items()}
        rec["tensors_equal"] = all(torch.equal(x, y) for x, y in zip(got["now"], got["before"]))
        a, b = rec["png_decode_device_batch(rgba8)"], rec["png_decode_device_batch(rgba8) (before)"]
        rec["difference_ms"] = round(a["best_ms"] - b["best_ms"], 2)
        rec["allowed_ms"] = round(a["spread_ms"] + b["spread_ms"], 2)
        out[name + ", existing"] = rec
        del arena
    return out


TABLES = {"kernels": _kernels, "calls": _calls}


def _child(table, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", table, "--repeat", str(args.repeat), "--size", str(args.size),
           "--icons", str(args.icons)] + (["--parent-lib", args.parent_lib] if args.parent_lib else [])
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{table}: {r.stderr[-3000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def _line(name, s, extra=""):
    print(f"  {name:<84}{s['best_ms']:>12.3f}{s['spread_ms']:>11.3f}{extra}")


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
    head = f"  {'':<84}{'best ms':>12}{'spread ms':>11}"
    results["kernels"] = ker = _child("kernels", args)
    print(f"(a) k_png_unpack alone (HIP events), best of {args.repeat} after a warm-up; stored = the chain's tensor computed on the host: {ker.pop('equal')}")
    print(head + "       GB/s")
    for name, rec in ker.items():
        for label, s in rec.items():
            if isinstance(s, dict):
                _line(f"{name}: {label}", s, f"{s['GB/s']:>11.1f}")
        print(f"    ({rec['read']} bytes read, {rec['written']} written: {'inside' if rec['inside_cache'] else 'larger than'} the {CACHE_MB} MB Infinity Cache)")
    results["calls"] = calls = _child("calls", args)
    against = "the parent commit's library" if calls.pop("parent_library") else "this library"
    print(f"\n(b), (c) the calls (wall, one process, ways alternating) on {args.icons} icon files of 64 x 64; 'before' is {against}'s")
    for name, rec in calls.items():
        print(f"  {name}")
        print(head)
        for way, s in rec.items():
            if isinstance(s, dict):
                _line(way, s)
        if "values_differing" in rec:
            print(f"    values that differ from the device-side chain: {rec['values_differing']}, by at most {rec['max_abs_difference']:.3g}; "
                  f"equal to the chain computed on the host: {rec['equal_to_the_chain_on_the_host']}")
        print(f"    the tensors are equal: {rec['tensors_equal']}; new - before = {rec['difference_ms']} ms; both spreads = {rec['allowed_ms']} ms"
              + (f": {'holds' if rec['difference_ms'] <= rec['allowed_ms'] else 'DOES NOT HOLD'}" if name.endswith("existing") else ""))
    print()
    print(json.dumps({"repeat": args.repeat, "size": args.size, "icons": args.icons, "parent_lib": against != "this library", "results": results}))


if __name__ == "__main__":
    main()
