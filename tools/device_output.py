"""Output left in device memory: what zmx_compress_device_to_device costs beside zmx_compress_device, and k_bitjoin alone.

(a) One input of class T in device memory (100 MB by default), numiterations 15, gzip, with and without block splitting:
    zmx_compress_device_to_device of this build against zmx_compress_device of this build and, with --parent-lib, of the
    parent commit's library (tools/build_variant.py builds one from a checkout of it).  Every way runs in a process of its
    own — two libraries in one process would share the device's memory between their context pools — as a warm-up call and
    --repeat timed calls; the table gives the best and the spread (max - min) of each.
(b) zmx_bitjoin_device alone, by HIP events (zmx_internal_bitjoin_ms): the join inside the call, on the stream's own
    piece table; then a table of the stream's shape over a copy of the stream — as many blocks as the call reported, each
    a header piece of 4096 bits and its share of the bits — with sources and destination congruent mod 32 bits and with
    every source one bit off; beside one hipMemcpyAsync device to device of the same bytes.

usage: python tools/device_output.py [--mb 100] [--repeat 5] [--parent-lib PATH]       prints a table and one JSON line
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _runs(entry, nbytes, repeat):
    """A child's work: `entry` on class T, blocksplitting 0 and 1; prints one JSON line."""
    import torch

    from zopfli_amd import ZopfliOptions, api, generate
    lib = api.library()
    lib.zmx_set_kernel_timing(0)     # (as any caller that does not ask for the phase times)
    data = generate("T", nbytes)
    src = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    out = {}
    for splitting in (0, 1):
        opt = ZopfliOptions(15, splitting, 15)
        if entry == "device_out":
            dst = torch.empty(api.compress_bound(nbytes), dtype=torch.uint8, device="cuda")
            call = lambda: api.compress_device_out(src, dst, api.FORMAT_GZIP, opt, lib=lib)   # noqa: E731
        else:
            call = lambda: len(api.compress_device(src, fmt=api.FORMAT_GZIP, options=opt, lib=lib))   # noqa: E731
        torch.cuda.synchronize()
        size = call()      # (warm: the contexts exist, the pools hold their arrays)
        ms = []
        for _ in range(repeat):
            t0 = time.perf_counter()
            call()
            ms.append((time.perf_counter() - t0) * 1e3)
        rec = {"ms": [round(m, 2) for m in ms], "stream_bytes": size}
        if entry == "device_out":
            rec["output_traffic"] = api.last_output_traffic(lib)
            rec["join"] = _join_alone(lib, src, dst, size, rec["output_traffic"], splitting)
        out[f"blocksplitting={splitting}"] = rec
    print(json.dumps(out), flush=True)


def _join_alone(lib, src, dst, size, traffic, splitting):
    import torch

    from batch_files import _Hip
    from zopfli_amd import Context, ZopfliOptions, api
    lib.zmx_internal_bitjoin_ms.restype = ctypes.c_double
    hip = _Hip()
    out = {}
    # the join inside the call (the calling thread makes it), events on
    lib.zmx_set_kernel_timing(1)
    best = None
    for _ in range(3):
        # (numiterations 1: the parse is not what is measured here; the piece table has the same shape)
        n = api.compress_device_out(src, dst, api.FORMAT_GZIP, ZopfliOptions(1, splitting, 15), lib=lib)
        ms = lib.zmx_internal_bitjoin_ms()
        best = ms if best is None else min(best, ms)
    out["inside_the_call"] = {"ms": round(best, 4), "GB/s": round(n / 1e9 / (best / 1e3), 1), "stream_bytes": n}
    blocks = max(1, int(traffic[2] + traffic[3]))
    stream = dst[:size].clone()
    spare = torch.empty(size + 64, dtype=torch.uint8, device="cuda")
    total_bits = 8 * size
    ctx = Context(0, lib)
    try:
        for name, off in (("co_aligned", 0), ("one_bit_off", 1)):
            pieces, at = [], 0
            share = (total_bits - off) // blocks
            for b in range(blocks):
                end = total_bits - off if b + 1 == blocks else at + share
                head = min(4096, end - at)
                pieces.append((stream.data_ptr(), at + off, head, at))
                if end > at + head:
                    pieces.append((stream.data_ptr(), at + head + off, end - at - head, at + head))
                at = end
            torch.cuda.synchronize()
            ctx.bitjoin_device(pieces, total_bits, spare.data_ptr(), size)   # (warm)
            ms = None
            for _ in range(5):
                ctx.bitjoin_device(pieces, total_bits, spare.data_ptr(), size)
                m = lib.zmx_internal_bitjoin_ms()
                ms = m if ms is None else min(ms, m)
            right = bool(torch.equal(spare[:size - 1], stream[:size - 1])) if off == 0 else None
            out[name] = {"pieces": len(pieces), "ms": round(ms, 4), "GB/s": round(size / 1e9 / (ms / 1e3), 1), "equals_the_stream": right}
        hip.copies_ms(spare.data_ptr(), [(stream.data_ptr(), size)])    # (warm)
        one = min(hip.copies_ms(spare.data_ptr(), [(stream.data_ptr(), size)]) for _ in range(5))
        out["one_hipMemcpyAsync"] = {"ms": round(one, 4), "GB/s": round(size / 1e9 / (one / 1e3), 1)}
    finally:
        lib.zmx_set_kernel_timing(0)
        ctx.close()
    return out


def _child(entry, nbytes, repeat, lib_path=None):
    env = dict(os.environ)
    if lib_path:
        env["ZOPFLI_AMD_LIB"] = lib_path
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", entry, "--mb", str(nbytes / 1e6), "--repeat", str(repeat)],
                       env=env, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{entry}: {r.stderr[-3000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=100)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libzopfli_amd.so of the parent commit")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    nbytes = int(args.mb * 1e6)
    if args.child:
        _runs(args.child, nbytes, args.repeat)
        return
    ways = [("zmx_compress_device_to_device", "device_out", None), ("zmx_compress_device", "device", None)]
    if args.parent_lib:
        ways.append(("zmx_compress_device, parent commit", "device", os.path.abspath(args.parent_lib)))
    results = {name: _child(entry, nbytes, args.repeat, path) for name, entry, path in ways}
    print(f"{args.mb:g} MB of class T in device memory, numiterations 15, gzip; a warm-up call, then {args.repeat} timed calls (ms)")
    for key in ("blocksplitting=0", "blocksplitting=1"):
        print(f"\n{key}")
        print(f"  {'entry':<40}{'best':>9}{'spread':>9}   runs")
        for name, _, _ in ways:
            ms = results[name][key]["ms"]
            print(f"  {name:<40}{min(ms):>9.2f}{max(ms) - min(ms):>9.2f}   {ms}")
        rec = results["zmx_compress_device_to_device"][key]
        print(f"  stream {rec['stream_bytes']} bytes; output traffic [down, up, device blocks, host blocks] = {rec['output_traffic']}")
        for name, j in rec["join"].items():
            print(f"  k_bitjoin {name:<20} {json.dumps(j)}")
        if args.parent_lib:
            new = min(rec["ms"])
            parent = results["zmx_compress_device, parent commit"][key]["ms"]
            holds = new <= min(parent) + (max(parent) - min(parent))
            print(f"  not slower than the parent by more than the parent's spread: {'holds' if holds else 'DOES NOT HOLD'} "
                  f"({new:.2f} against {min(parent):.2f} + {max(parent) - min(parent):.2f})")
    print()
    print(json.dumps({"mb": args.mb, "repeat": args.repeat, "results": results}))


if __name__ == "__main__":
    main()
