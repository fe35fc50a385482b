"""PNG decode on the device: what zmx_png_decode_device_batch costs beside what a caller who holds PNG files in device memory
does today.

Three sets, decoded to RGBA8: 1 000 icons of 64 x 64 RGBA8 from png_encode_device_batch_packed at strategy e (numiterations
2), the same icons of 16 colours as palette files (png_optimize_device_batch, uploaded as they are), and one 4096 x 4096
RGBA8 file (zlib level 6 on the host, uploaded).  One MI355X, one process a set (a table each).  Per set, after a warm-up of
every way, the ways alternate --repeat times; the table gives the best and the spread (max - min) of each:
  k_png_chunks and k_png_unfilter alone, by HIP events inside the call (zmx_internal_png_decode_ms), beside one device to
  device copy of the pixels (torch events);
  the call's wall time and its split by the host's clock (zmx_internal_png_decode_phase_ms): the walk, the CRCs, the gather
  and k_inflate, the Adler-32s, the unfilter;
  today: the files device to host, PIL on one thread or on sixteen, the pixels host to device (wall).
All outputs are compared with the images on the device.

usage: python tools/png_decode.py [--repeat 5] [--out profiles/png_decode.txt]       prints the tables and one JSON line
"""
import argparse
import concurrent.futures
import ctypes
import io
import json
import os
import struct
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETS = ["1000 icons 64 x 64 RGBA8", "1000 icons 64 x 64 palette", "1 x 4096 x 4096 RGBA8"]
PHASES = ["walk", "CRC-32s", "gather + k_inflate", "Adler-32s", "unfilter"]


def _icons(np, count, colours):
    rng = np.random.default_rng(1)
    y, x = np.mgrid[0:64, 0:64]
    out = []
    for i in range(count):
        if colours:
            table = rng.integers(0, 256, size=(colours, 4), dtype=np.uint8)
            out.append(table[((x // 4 + y // 3 + i) ^ (x * y // 97)) % colours])
        else:
            base = np.stack([(3 * x + i) & 255, (2 * y + 5 * i) & 255, (x + y) & 255, 255 - ((x * y) >> 4 & 255)], axis=2)
            out.append(((base + rng.integers(-2, 3, size=base.shape)) & 255).astype(np.uint8))
    return out


def _host_png(np, img):
    h, w, _ = img.shape
    # (filter type 1 with bytewidth 4: the difference to the pixel on the left)
    scan = np.empty((h, 1 + w * 4), dtype=np.uint8)
    scan[:, 0] = 1
    flat = img.reshape(h, w * 4).astype(np.int16)
    left = np.concatenate([np.zeros((h, 4), dtype=np.int16), flat[:, :-4]], axis=1)
    scan[:, 1:] = ((flat - left) & 255).astype(np.uint8)

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xffffffff)
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(scan.tobytes(), 6)) +
            chunk(b"IEND", b""))


def _child(name, repeat):
    import numpy as np
    import torch
    from PIL import Image

    from zopfli_amd import ZopfliOptions, api
    lib = api.library()
    Image.MAX_IMAGE_PIXELS = None
    if name == SETS[0]:
        imgs = [torch.from_numpy(a).cuda() for a in _icons(np, 1000, 0)]
        arena = torch.empty(api.png_batch_bound(imgs, 16, lib=lib), dtype=torch.uint8, device="cuda")
        offsets, sizes = api.png_encode_device_batch_packed(imgs, arena, 16, "e", ZopfliOptions(2), lib=lib)
    else:
        if name == SETS[1]:
            imgs = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in _icons(np, 1000, 16)]
            made = api.png_optimize_device_batch(imgs, "e", ZopfliOptions(2), lib=lib)
        else:
            y, x = np.mgrid[0:4096, 0:4096]
            big = np.stack([(x + y) & 255, (x * 3 >> 2) & 255, (y * 5 >> 3) & 255, 255 - ((x ^ y) & 255)], axis=2).astype(np.uint8)
            imgs = [torch.from_numpy(big).cuda()]
            made = [_host_png(np, big)]
        offsets, sizes, blob = [], [], bytearray()
        for f in made:
            blob += bytes(-len(blob) % 16)
            offsets.append(len(blob))
            sizes.append(len(f))
            blob += bytes(f)
        arena = torch.frombuffer(blob, dtype=torch.uint8).cuda()
    files = [(arena.data_ptr() + o, s) for o, s in zip(offsets, sizes)]
    pixels = sum(int(im.numel()) for im in imgs)
    whole = torch.cat([im.reshape(-1) for im in imgs])
    back = torch.zeros(pixels, dtype=torch.uint8, device="cuda")
    outs, at = [], 0
    for im in imgs:
        outs.append(back[at:at + im.numel()])
        at += im.numel()
    torch.cuda.synchronize()
    kernels, phases = {"k_png_chunks (events)": [], "k_png_unfilter (events)": []}, {p: [] for p in PHASES}
    ms2, ms5 = (ctypes.c_double * 2)(), (ctypes.c_double * 5)()

    def device_way():
        api.png_decode_device_batch(files, "rgba8", outs, lib=lib)
        lib.zmx_internal_png_decode_ms(ms2)
        lib.zmx_internal_png_decode_phase_ms(ms5)
        kernels["k_png_chunks (events)"].append(ms2[0])
        kernels["k_png_unfilter (events)"].append(ms2[1])
        for p, v in zip(PHASES, ms5):
            phases[p].append(v)

    def copy_way():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        back.copy_(whole)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def host_way(threads):
        def way():
            host = arena.cpu().numpy()
            pieces = [host[o:o + s].tobytes() for o, s in zip(offsets, sizes)]
            decode = lambda p: Image.open(io.BytesIO(p)).convert("RGBA").tobytes()   # noqa: E731
            if threads == 1:
                made = [decode(p) for p in pieces]
            else:
                with concurrent.futures.ThreadPoolExecutor(threads) as pool:
                    made = list(pool.map(decode, pieces))
            up = torch.frombuffer(bytearray(b"".join(made)), dtype=torch.uint8).cuda()
            torch.cuda.synchronize()
            return up
        return way

    ways = {"zmx_png_decode_device_batch, the call (wall)": device_way, "today: D2H, PIL on 1 thread, H2D (wall)": host_way(1),
            "today: D2H, PIL on 16 threads, H2D (wall)": host_way(16)}
    equal = {}
    for label, way in ways.items():      # the warm-up, and the check
        back.zero_()
        made = way()
        equal[label] = bool(torch.equal(back if made is None else made, whole))
    modes = sorted({(int(r.colortype), int(r.bitdepth)) for r in api.png_info_device(files, lib=lib)})
    copy_way()
    for runs in list(kernels.values()) + list(phases.values()):
        runs.clear()
    ms = {label: [] for label in ways}
    copies = []
    for _ in range(repeat):
        for label, way in ways.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            way()
            ms[label].append((time.perf_counter() - t0) * 1e3)
        copies.append(copy_way())
    first = next(iter(ways))
    table = {**kernels, "one device to device copy of the pixels (events)": copies, first: ms[first],
             **{"  of it: " + p: v for p, v in phases.items()}, **{k: v for k, v in ms.items() if k != first}}
    print(json.dumps({"files": len(files), "pixel_bytes": pixels, "file_bytes": sum(sizes), "modes": modes, "equal": equal,
                      "ms": {k: [round(v, 4) for v in vs] for k, vs in table.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--sets", default=None, help="comma-separated indices of the sets to run (default: all)")
    args = ap.parse_args()
    if args.child:
        return _child(args.child, args.repeat)
    names = SETS if args.sets is None else [SETS[int(i)] for i in args.sets.split(",")]
    lines, results = [f"PNG decode on the device, to RGBA8; one process a set, the ways alternate, best of {args.repeat} after a warm-up", ""], {}
    for name in names:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--repeat", str(args.repeat)], capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            return 1
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        results[name] = rec
        lines.append(f" {name}: {rec['file_bytes']} bytes of files, {rec['pixel_bytes']} bytes of pixels, colour type and depth {rec['modes']}; outputs equal the images: {all(rec['equal'].values())}")
        lines.append(f"  {'':70s} {'best ms':>10s} {'spread ms':>10s} {'GB/s':>10s}")
        for label, runs in rec["ms"].items():
            best = min(runs)
            lines.append(f"  {label:70s} {best:10.3f} {max(runs) - best:10.3f} {rec['pixel_bytes'] / 1e9 / (max(best, 1e-6) / 1e3):10.3f}")
        lines.append("")
        print("\n".join(lines[-(len(rec["ms"]) + 3):]), flush=True)
    lines.append(json.dumps({"repeat": args.repeat, "results": results}))
    print(lines[-1])
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
