"""Inflate on the device: what zmx_inflate_device_batch costs beside what a caller of the *_to_device entries does today.

Three sets of class T streams made by compress_device_batch_packed at numiterations 15 (gzip): 1 000 x 64 KiB, 200 x 1 MB
and one 100 MB stream.  One MI355X, one process a set (a table each).  Per set, after a warm-up of every way, the ways
alternate --repeat times; the table gives the best and the spread (max - min) of each:
  k_inflate alone, by HIP events (zmx_internal_inflate_ms) inside the call, in ms and GB/s of output;
  zmx_inflate_device_batch, the call (wall): k_inflate, the results down, the checksum kernels, their values down;
  today: the streams device to host, zlib.decompress of each on one thread or on sixteen, the outputs host to device (wall).
All outputs are compared with the inputs on the device.

usage: python tools/inflate_device.py [--repeat 5] [--out profiles/inflate_device.txt]       prints the tables and one JSON line
"""
import argparse
import concurrent.futures
import ctypes
import json
import os
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETS = {"1000 x 64 KiB": (1000, 65536), "200 x 1 MB": (200, 1000000), "1 x 100 MB": (1, 100000000)}


def _child(name, repeat):
    import torch

    from zopfli_amd import ZopfliOptions, api, generate
    lib = api.library()
    lib.zmx_internal_inflate_ms.restype = ctypes.c_double
    count, each = SETS[name]
    whole = torch.frombuffer(bytearray(generate("T", count * each)), dtype=torch.uint8).cuda()
    srcs = [whole[i * each:(i + 1) * each] for i in range(count)]
    arena = torch.empty(api.compress_batch_bound([each] * count, api.FORMAT_GZIP, 1, lib=lib), dtype=torch.uint8, device="cuda")
    offsets, sizes = api.compress_device_batch_packed(srcs, arena, 1, api.FORMAT_GZIP, ZopfliOptions(15), lib=lib)
    streams = [(arena.data_ptr() + o, s) for o, s in zip(offsets, sizes)]
    back = torch.zeros(count * each, dtype=torch.uint8, device="cuda")
    outs = [back[i * each:(i + 1) * each] for i in range(count)]
    torch.cuda.synchronize()
    kernel_ms = []

    def device_way():
        api.inflate_device_batch(streams, "gzip", outs, lib=lib)
        kernel_ms.append(lib.zmx_internal_inflate_ms())

    def host_way(threads):
        def way():
            host = arena[:offsets[-1] + sizes[-1]].cpu().numpy()
            pieces = [host[o:o + s] for o, s in zip(offsets, sizes)]
            inflate = lambda p: zlib.decompress(p, 31)   # noqa: E731
            if threads == 1:
                made = [inflate(p) for p in pieces]
            else:
                with concurrent.futures.ThreadPoolExecutor(threads) as pool:
                    made = list(pool.map(inflate, pieces))
            up = torch.frombuffer(bytearray(b"".join(made)), dtype=torch.uint8).cuda()
            torch.cuda.synchronize()
            return up
        return way

    ways = {"zmx_inflate_device_batch, the call (wall)": device_way, "today: D2H, zlib on 1 thread, H2D (wall)": host_way(1),
            "today: D2H, zlib on 16 threads, H2D (wall)": host_way(16)}
    equal = {}
    for label, way in ways.items():      # the warm-up, and the check
        back.zero_()
        made = way()
        equal[label] = bool(torch.equal(back if made is None else made, whole))
    kernel_ms.clear()
    ms = {label: [] for label in ways}
    for _ in range(repeat):
        for label, way in ways.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            way()
            ms[label].append((time.perf_counter() - t0) * 1e3)
    ms = {"k_inflate (events)": kernel_ms, **ms}
    print(json.dumps({"streams": count, "output_bytes": count * each, "stream_bytes": sum(sizes), "equal": equal,
                      "ms": {k: [round(v, 4) for v in vs] for k, vs in ms.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        return _child(args.child, args.repeat)
    lines, results = [f"inflate on the device, class T, gzip streams of compress_device_batch_packed at numiterations 15; one process a set, the ways alternate, "
                      f"best of {args.repeat} after a warm-up", ""], {}
    for name in SETS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--repeat", str(args.repeat)], capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            return 1
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        results[name] = rec
        lines.append(f" {name}: {rec['stream_bytes']} bytes of streams, {rec['output_bytes']} bytes of output; outputs equal the inputs: {all(rec['equal'].values())}")
        lines.append(f"  {'':70s} {'best ms':>10s} {'spread ms':>10s} {'GB/s':>10s}")
        for label, runs in rec["ms"].items():
            best = min(runs)
            lines.append(f"  {label:70s} {best:10.3f} {max(runs) - best:10.3f} {rec['output_bytes'] / 1e9 / (best / 1e3):10.3f}")
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
