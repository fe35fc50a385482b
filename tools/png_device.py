"""An image in device memory as a PNG: what k_png_rows, zmx_png_encode_device and its batch cost.

Three tables, each measured in a child process of its own (nothing warmed by one table helps another); inside a
process the ways that are compared alternate, after a warm-up call of each, and a line gives the best of --repeat runs
and the spread (max - min).
(a) k_png_rows alone, by HIP events (zmx_internal_png_rows_ms), on a 4096 x 4096 RGBA8 image under the types the
    ENTROPY search picks and under each single type, and on 1 000 images of 64 x 64 RGBA8 (a launch each; the events'
    sum and the wall time of the 1 000 calls); beside one hipMemcpyAsync device to device of the scanlines' bytes.
    GB/s counts the algorithmic bytes: the image read once, the scanlines written once (the copy: the same bytes read and
    written).
(b) zmx_png_encode_device of the 4096 x 4096 image, strategy e, numiterations 5, against zmx_compress_device(ZLIB) of
    the already filtered scanlines in the same process, and the entry's own device work (zmx_png_filter_types_device +
    zmx_png_filter_rows_device, host clock around the two synchronous calls).
(c) zmx_png_encode_device_batch of 1 000 images of 64 x 64 RGBA8, numiterations 15, against 1 000 single calls and
    against zmx_compress_device_batch(ZLIB) of the filtered scanlines.
(d) with --cli: for information, the wall time of oracle/_ref/zopflipng_amd2 -y --always_zopflify --keepcolortype
    --filters=e on the 4096 x 4096 image as a file — process start, decoding and the file's way up included.

usage: python tools/png_device.py [--repeat 5] [--size 4096] [--icons 1000] [--cli]     prints the tables and one JSON line
"""
import argparse
import ctypes
import json
import os
import struct
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _image(w, seed=7):
    """tools/png_at_size.py's synthetic W x W RGBA image: a gradient with +-3 of noise."""
    import numpy as np
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:w, 0:w]
    img = np.stack([(x * 255 // max(w - 1, 1)), (y * 255 // max(w - 1, 1)), ((x + y) // 3 % 256), np.full_like(x, 255)],
                   axis=-1).astype(np.int32)
    img[..., :3] += rng.integers(-3, 4, size=(w, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def _stats(ms):
    return {"best_ms": round(min(ms), 4), "spread_ms": round(max(ms) - min(ms), 4), "runs": [round(m, 4) for m in ms]}


def _wall(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def _alternate(ways, repeat):
    """{name: [ms]} of the callables in `ways`, a warm-up of each and then `repeat` rounds through all of them."""
    for fn in ways.values():
        fn()
    ms = {name: [] for name in ways}
    for _ in range(repeat):
        for name, fn in ways.items():
            ms[name].append(_wall(fn))
    return ms


def _rows_alone(args):
    import torch

    from batch_files import _Hip
    from zopfli_amd import Context, api
    lib = api.library()
    lib.zmx_internal_png_rows_ms.restype = ctypes.c_double
    lib.zmx_set_kernel_timing(1)
    hip = _Hip()
    ctx = Context(0, lib)
    out = {}
    w = args.size
    n, h = 4 * w, w
    total = h * (n + 1)
    img = torch.from_numpy(_image(w)).cuda()
    types = torch.zeros(h, dtype=torch.uint8, device="cuda")
    scan = torch.empty(total, dtype=torch.uint8, device="cuda")
    spare = torch.empty(total, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    big = {}
    for name in ("e", "0", "1", "2", "3", "4"):
        ctx.png_filter_types_device(img, n, h, 4, name, types)
        ms = []
        for i in range(args.repeat + 1):
            ctx.png_filter_rows_device(img, n, h, 4, types, scan)
            copy = hip.copies_ms(spare.data_ptr(), [(scan.data_ptr(), total)])
            if i:      # (the first round is the warm-up)
                ms.append((lib.zmx_internal_png_rows_ms(), copy))
        rec = {"k_png_rows": _stats([m[0] for m in ms]), "one_hipMemcpyAsync": _stats([m[1] for m in ms])}
        rec["k_png_rows"]["GB/s"] = round((n * h + total) / 1e6 / rec["k_png_rows"]["best_ms"], 1)
        rec["one_hipMemcpyAsync"]["GB/s"] = round(2 * total / 1e6 / rec["one_hipMemcpyAsync"]["best_ms"], 1)
        if name == "e":
            rec["types_picked"] = [int(v) for v in torch.bincount(types.int(), minlength=5).cpu()]
        big["types " + name] = rec
    out[f"{w}x{w} RGBA8"] = {"image_bytes": n * h, "scanline_bytes": total, "fits_infinity_cache": n * h + total <= 256 << 20,
                             "ways": big}
    # ---- the icons: a launch each
    k, iw = args.icons, 64
    n, h = 4 * iw, iw
    total = h * (n + 1)
    icons = torch.from_numpy(_image(iw, 3)).cuda().repeat(k, 1, 1, 1).contiguous()
    types = torch.zeros(h, dtype=torch.uint8, device="cuda")
    ctx.png_filter_types_device(icons[0], n, h, 4, "e", types)
    scan = torch.empty(k * total, dtype=torch.uint8, device="cuda")
    spare = torch.empty(k * total, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    events, walls, copies = [], [], []
    for i in range(args.repeat + 1):
        t0 = time.perf_counter()
        ev = 0.0
        for j in range(k):
            ctx.png_filter_rows_device(icons[j].data_ptr(), n, h, 4, types, scan.data_ptr() + j * total, total)
            ev += lib.zmx_internal_png_rows_ms()
        wall = (time.perf_counter() - t0) * 1e3
        copy = hip.copies_ms(spare.data_ptr(), [(scan.data_ptr(), k * total)])
        if i:
            events.append(ev)
            walls.append(wall)
            copies.append(copy)
    rec = {"k_png_rows_events_sum": _stats(events), "calls_wall": _stats(walls), "one_hipMemcpyAsync": _stats(copies)}
    rec["k_png_rows_events_sum"]["GB/s"] = round(k * (n * h + total) / 1e6 / min(events), 1)
    rec["one_hipMemcpyAsync"]["GB/s"] = round(2 * k * total / 1e6 / min(copies), 1)
    out[f"{k} x {iw}x{iw} RGBA8"] = {"image_bytes": k * n * h, "scanline_bytes": k * total, "fits_infinity_cache": True, "ways": rec}
    ctx.close()
    return out


def _encode_big(args):
    import torch

    from zopfli_amd import Context, ZopfliOptions, api
    lib = api.library()
    lib.zmx_set_kernel_timing(0)
    w = args.size
    n, h = 4 * w, w
    total = h * (n + 1)
    img = torch.from_numpy(_image(w)).cuda()
    types = torch.zeros(h, dtype=torch.uint8, device="cuda")
    scan = torch.empty(total, dtype=torch.uint8, device="cuda")
    ctx = Context(0, lib)
    opt = ZopfliOptions(5)
    sizes = {}

    def own_kernels():
        ctx.png_filter_types_device(img, n, h, 4, "e", types)
        ctx.png_filter_rows_device(img, n, h, 4, types, scan)

    own_kernels()
    torch.cuda.synchronize()

    def encode():
        sizes["png"] = len(api.png_encode_device(img, "e", opt, lib=lib))

    def compress():
        sizes["zlib"] = len(api.compress_device(scan, fmt=api.FORMAT_ZLIB, options=opt, lib=lib))

    ms = _alternate({"zmx_png_encode_device": encode, "zmx_compress_device(ZLIB) of the scanlines": compress,
                     "types + rows on the device": own_kernels}, args.repeat)
    ctx.close()
    out = {name: _stats(v) for name, v in ms.items()}
    e, c, k = (out[name] for name in ms)
    out["difference_ms"] = round(e["best_ms"] - c["best_ms"], 2)
    out["allowed_ms"] = round(k["best_ms"] + e["spread_ms"] + c["spread_ms"], 2)
    out["bytes"] = sizes
    return out


def _encode_icons(args):
    import torch

    from zopfli_amd import Context, ZopfliOptions, api
    lib = api.library()
    lib.zmx_set_kernel_timing(0)
    k, iw = args.icons, 64
    n, h = 4 * iw, iw
    total = h * (n + 1)
    # (every icon its own noise: equal files would flatter nothing here, but they would be no batch a user has)
    icons = [torch.from_numpy(_image(iw, 100 + i)).cuda() for i in range(k)]
    scan = torch.empty(k * total, dtype=torch.uint8, device="cuda")
    types = torch.zeros(h, dtype=torch.uint8, device="cuda")
    ctx = Context(0, lib)
    for i in range(k):
        ctx.png_filter_types_device(icons[i], n, h, 4, "e", types)
        ctx.png_filter_rows_device(icons[i], n, h, 4, types, scan.data_ptr() + i * total, total)
    ctx.close()
    torch.cuda.synchronize()
    opt = ZopfliOptions(15)
    got = {}

    def batch():
        got["batch"] = api.png_encode_device_batch(icons, "e", opt, lib=lib)

    def singles():
        got["singles"] = [api.png_encode_device(t, "e", opt, lib=lib) for t in icons]

    def compress_batch():
        got["zlib"] = api.compress_device_batch([(scan.data_ptr() + i * total, total) for i in range(k)], api.FORMAT_ZLIB, opt, lib=lib)

    ms = _alternate({"zmx_png_encode_device_batch": batch, f"{k} x zmx_png_encode_device": singles,
                     "zmx_compress_device_batch(ZLIB) of the scanlines": compress_batch}, args.repeat)
    out = {name: _stats(v) for name, v in ms.items()}
    out["batch_equals_singles"] = got["batch"] == got["singles"]
    out["bytes"] = {"png": sum(len(p) for p in got["batch"]), "zlib": sum(len(z) for z in got["zlib"])}
    return out


def _cli(args):
    from zopfli_amd._build import PNG_AMD2
    import tempfile
    w = args.size
    img = _image(w)
    import numpy as np
    raw = np.concatenate([np.zeros((w, 1), dtype=np.uint8), img.reshape(w, w * 4)], axis=1).tobytes()

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)

    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in.png"), os.path.join(d, "out.png")
        with open(src, "wb") as f:
            f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, w, 8, 6, 0, 0, 0)) +
                    chunk(b"IDAT", zlib.compress(raw, 1)) + chunk(b"IEND", b""))
        t0 = time.perf_counter()
        r = subprocess.run([PNG_AMD2, "-y", "--always_zopflify", "--keepcolortype", "--filters=e", src, dst], capture_output=True, text=True)
        wall = time.perf_counter() - t0
        if r.returncode != 0:
            raise RuntimeError(r.stdout[-1000:] + r.stderr[-1000:])
        return {"wall_s_including_process_start": round(wall, 2), "bytes": os.path.getsize(dst)}


TABLES = {"rows": _rows_alone, "encode": _encode_big, "icons": _encode_icons, "cli": _cli}


def _child(table, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", table, "--repeat", str(args.repeat), "--size", str(args.size),
           "--icons", str(args.icons)]
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
    ap.add_argument("--cli", action="store_true")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(TABLES[args.child](args)), flush=True)
        return
    results = {}
    head = f"  {'':<52}{'best ms':>12}{'spread ms':>11}"
    results["rows"] = rows = _child("rows", args)
    print(f"(a) k_png_rows alone (HIP events), best of {args.repeat} after a warm-up")
    for shape, rec in rows.items():
        print(f"\n {shape}: image {rec['image_bytes']} bytes, scanlines {rec['scanline_bytes']} bytes; read + written "
              f"{'fit' if rec['fits_infinity_cache'] else 'do not fit'} the 256 MiB Infinity Cache")
        print(head + "       GB/s")
        ways = rec["ways"]
        if "calls_wall" in ways:
            ways = {"": ways}
        for types, w in ways.items():
            for name, s in w.items():
                if isinstance(s, dict):
                    _line((types + ": " if types else "") + name, s, f"{s['GB/s']:>11.1f}" if "GB/s" in s else "")
            if "types_picked" in w:
                print(f"    (rows of type 0..4 under e: {w['types_picked']})")
    results["encode"] = enc = _child("encode", args)
    print(f"\n(b) {args.size} x {args.size} RGBA8, strategy e, numiterations 5 (wall, one process, ways alternating)")
    print(head)
    for name, s in enc.items():
        if isinstance(s, dict) and "best_ms" in s:
            _line(name, s)
    print(f"  entry - compress = {enc['difference_ms']} ms; allowed: own device work + both spreads = {enc['allowed_ms']} ms: "
          f"{'holds' if enc['difference_ms'] <= enc['allowed_ms'] else 'DOES NOT HOLD'};  bytes {enc['bytes']}")
    results["icons"] = ico = _child("icons", args)
    print(f"\n(c) {args.icons} x 64 x 64 RGBA8, strategy e, numiterations 15 (wall, one process, ways alternating)")
    print(head)
    for name, s in ico.items():
        if isinstance(s, dict) and "best_ms" in s:
            _line(name, s)
    print(f"  the batch's files equal the single calls': {ico['batch_equals_singles']};  bytes {ico['bytes']}")
    if args.cli:
        results["cli"] = cli = _child("cli", args)
        print(f"\n(d) for information: zopflipng_amd2 -y --always_zopflify --keepcolortype --filters=e on the {args.size} x {args.size} "
              f"image as a file: {cli['wall_s_including_process_start']} s wall, process start included ({cli['bytes']} bytes)")
    print()
    print(json.dumps({"repeat": args.repeat, "size": args.size, "icons": args.icons, "results": results}))


if __name__ == "__main__":
    main()
