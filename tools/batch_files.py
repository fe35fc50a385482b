"""Many small files: one zmx_compress_batch call against the 16-caller ZopfliCompress loop, in the same process.

The two sets of bench.py's `small_files` line — 1000 x 64 KiB and 200 x 1 MB, classes T and X alternating (seeds 1000 ...),
the reference's default options with numiterations = 15, gzip.  For each set: MB/s of one batch call (after a warm-up batch),
MB/s of 16 caller threads each calling ZopfliCompress on one file at a time (after a warm-up round), and whether every
batch output equals the single call's.  Prints one JSON line.

--device: the same sets as tensors in device memory, four ways in one process — one zmx_compress_device_batch call, the
16-caller loop of zmx_compress_device (all there was before the device batch), zmx_compress_batch of host copies, and
zmx_gather_device alone (HIP events) beside one hipMemcpyAsync of the same total and n hipMemcpyAsync calls, with
co-aligned sources and with sources 1 byte off.  The outputs of the three compressing ways are compared.

usage: python tools/batch_files.py [--sets 1000x65536,200x1000000] [--callers 16] [--repeat 2] [--device]
"""
import argparse
import concurrent.futures as cf
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zopfli_amd import ZopfliOptions, api, generate  # noqa: E402

MB = 1e6


def _best(repeat, fn):
    best, out = None, None
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, out


class _Hip:
    """The few runtime calls the copy baselines need, on the null stream, timed with HIP events."""

    def __init__(self):
        import ctypes
        self.c = ctypes
        # (the runtime this process has loaded already, torch's and the library's: not a second one)
        with open("/proc/self/maps") as f:
            paths = [line.split()[-1] for line in f if "libamdhip64" in line]
        self.hip = ctypes.CDLL(paths[0])
        self.hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
        self.hip.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self.hip.hipEventSynchronize.argtypes = [ctypes.c_void_p]
        self.hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
        self.ev = [ctypes.c_void_p(), ctypes.c_void_p()]
        for e in self.ev:
            assert self.hip.hipEventCreate(ctypes.byref(e)) == 0

    def copies_ms(self, dst, pairs):
        """Milliseconds (events) of one hipMemcpyAsync device to device per (pointer, nbytes) pair, end to end at dst."""
        assert self.hip.hipEventRecord(self.ev[0], None) == 0
        at = dst
        for ptr, n in pairs:
            assert self.hip.hipMemcpyAsync(at, ptr, n, 3, None) == 0    # hipMemcpyDeviceToDevice
            at += n
        assert self.hip.hipEventRecord(self.ev[1], None) == 0
        assert self.hip.hipEventSynchronize(self.ev[1]) == 0
        ms = self.c.c_float(0)
        assert self.hip.hipEventElapsedTime(self.c.byref(ms), self.ev[0], self.ev[1]) == 0
        return ms.value


def _gather_rates(lib, hip, files, repeat):
    """GB/s of zmx_gather_device, of one copy of the same total and of n copies; sources co-aligned and 1 byte off."""
    import ctypes

    import torch

    from zopfli_amd import Context
    total = sum(len(f) for f in files)
    lib.zmx_internal_gather_ms.restype = ctypes.c_double
    ctx = Context(0, lib)
    lib.zmx_set_kernel_timing(1)     # (the gather's events are taken only when asked for)
    out = {}
    try:
        for name, shift in (("co_aligned", 0), ("one_byte_off", 1)):
            # every source at a 256-byte boundary (+ shift) of one arena; the destination's pieces fall where the sizes put them
            offsets, at = [], 0
            for f in files:
                at = (at + 255) // 256 * 256
                offsets.append(at + shift)
                at += shift + len(f)
            arena = torch.empty(at, dtype=torch.uint8, device="cuda:0")
            for f, o in zip(files, offsets):
                arena[o:o + len(f)].copy_(torch.frombuffer(bytearray(f), dtype=torch.uint8))
            dst = torch.empty(total, dtype=torch.uint8, device="cuda:0")
            pairs = [(arena.data_ptr() + o, len(f)) for f, o in zip(files, offsets)]
            torch.cuda.synchronize()
            ctx.gather_device(pairs, dst)    # (warm)
            want = torch.cat([arena[o:o + len(f)] for f, o in zip(files, offsets)])
            equal = bool(torch.equal(dst, want))
            kernel_ms, wall_ms = None, None
            for _ in range(max(repeat, 3)):
                t0 = time.perf_counter()
                ctx.gather_device(pairs, dst)
                wall = (time.perf_counter() - t0) * 1e3
                ms = lib.zmx_internal_gather_ms()
                kernel_ms = ms if kernel_ms is None else min(kernel_ms, ms)
                wall_ms = wall if wall_ms is None else min(wall_ms, wall)
            hip.copies_ms(dst.data_ptr(), [(want.data_ptr(), total)])    # (warm)
            one_ms = min(hip.copies_ms(dst.data_ptr(), [(want.data_ptr(), total)]) for _ in range(max(repeat, 3)))
            n_ms = min(hip.copies_ms(dst.data_ptr(), pairs) for _ in range(max(repeat, 3)))
            gbs = lambda ms: round(total / 1e9 / (ms / 1e3), 2) if ms else None   # noqa: E731
            out[name] = {"equals_torch_cat": equal, "gather_events": {"GB/s": gbs(kernel_ms), "ms": round(kernel_ms, 4)},
                         "gather_call_wall": {"GB/s": gbs(wall_ms), "ms": round(wall_ms, 4)},
                         "one_hipMemcpyAsync": {"GB/s": gbs(one_ms), "ms": round(one_ms, 4)},
                         "n_hipMemcpyAsync": {"GB/s": gbs(n_ms), "ms": round(n_ms, 4), "n": len(pairs)}}
            del arena, dst, want
    finally:
        lib.zmx_set_kernel_timing(0)
        ctx.close()
    return out


def device_main(args, lib, opts):
    import torch
    hip = _Hip()
    line = {"metric": "many inputs in device memory: one zmx_compress_device_batch call vs %d zmx_compress_device callers vs "
                      "zmx_compress_batch of host copies" % args.callers,
            "options": "blocksplitting=1, blocksplittingmax=15, numiterations=15, gzip", "sets": []}
    for spec in args.sets.split(","):
        count, size = (int(x) for x in spec.split("x"))
        files = [generate("TX"[i & 1], size, seed=1000 + i) for i in range(count)]
        tensors = [torch.frombuffer(bytearray(f), dtype=torch.uint8).cuda() for f in files]
        torch.cuda.synchronize()
        total = count * size / MB

        def one(t):
            return api.compress_device(t, fmt=api.FORMAT_GZIP, options=opts, lib=lib)

        with cf.ThreadPoolExecutor(args.callers) as ex:
            list(ex.map(one, tensors[:2 * args.callers]))     # (warm: the callers' contexts exist)
            best_loop, single = _best(args.repeat, lambda: list(ex.map(one, tensors)))
        api.compress_device_batch(tensors[:64], api.FORMAT_GZIP, opts, lib=lib)   # (warm: the dealing contexts exist)
        best_dev, dev = _best(args.repeat, lambda: api.compress_device_batch(tensors, api.FORMAT_GZIP, opts, lib=lib))
        traffic = api.last_input_traffic(lib)
        best_host, host = _best(args.repeat, lambda: api.compress_batch(files, api.FORMAT_GZIP, opts, lib=lib))
        rec = {"files": count, "bytes_each": size, "classes": "T and X alternating, seeds 1000 ...",
               "device_batch": {"value": round(total / best_dev, 3), "unit": "MB/s", "ms": round(best_dev * 1e3, 1)},
               "device_callers_loop": {"value": round(total / best_loop, 3), "unit": "MB/s", "ms": round(best_loop * 1e3, 1),
                                       "callers": args.callers},
               "host_batch": {"value": round(total / best_host, 3), "unit": "MB/s", "ms": round(best_host * 1e3, 1)},
               "device_batch_over_loop": round(best_loop / best_dev, 2),
               "device_batch_over_host_batch": round(best_host / best_dev, 3),
               "input_traffic_of_device_batch": traffic,
               "outputs_equal": dev == single and dev == host,
               "gather": _gather_rates(lib, hip, files, args.repeat)}
        line["sets"].append(rec)
        print(json.dumps(rec), file=sys.stderr, flush=True)
        del tensors
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="1000x65536,200x1000000")
    ap.add_argument("--callers", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=2, help="timed repetitions of each way (the best counts)")
    ap.add_argument("--device", action="store_true", help="the sets as tensors in device memory (see above)")
    args = ap.parse_args()
    if args.device:
        import torch  # noqa: F401  (before the library: both then share torch's HIP runtime, and its tensors are device memory to the library)
    lib = api.library()
    lib.zmx_set_kernel_timing(0)     # (as any caller that does not ask for the phase times)
    opts = ZopfliOptions(15, 1, 15)
    if args.device:
        line = device_main(args, lib, opts)
        lib.zmx_set_kernel_timing(1)
        print(json.dumps(line), flush=True)
        return
    line = {"metric": "many small files, one batch call vs %d ZopfliCompress callers" % args.callers,
            "options": "blocksplitting=1, blocksplittingmax=15, numiterations=15, gzip", "sets": []}
    for spec in args.sets.split(","):
        count, size = (int(x) for x in spec.split("x"))
        files = [generate("TX"[i & 1], size, seed=1000 + i) for i in range(count)]
        total = count * size / MB

        def one(d):
            return api.compress(d, api.FORMAT_GZIP, opts, lib=lib)

        with cf.ThreadPoolExecutor(args.callers) as ex:
            list(ex.map(one, files[:2 * args.callers]))     # (warm: the callers' contexts exist)
            best_loop, single = None, None
            for _ in range(args.repeat):
                t0 = time.perf_counter()
                single = list(ex.map(one, files))
                dt = time.perf_counter() - t0
                best_loop = dt if best_loop is None else min(best_loop, dt)
        api.compress_batch(files[:64], api.FORMAT_GZIP, opts, lib=lib)   # (warm: the dealing contexts exist)
        best_batch, batch = None, None
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            batch = api.compress_batch(files, api.FORMAT_GZIP, opts, lib=lib)
            dt = time.perf_counter() - t0
            best_batch = dt if best_batch is None else min(best_batch, dt)
        rec = {"files": count, "bytes_each": size, "classes": "T and X alternating, seeds 1000 ...",
               "batch": {"value": round(total / best_batch, 3), "unit": "MB/s", "ms": round(best_batch * 1e3, 1)},
               "callers_loop": {"value": round(total / best_loop, 3), "unit": "MB/s", "ms": round(best_loop * 1e3, 1),
                                "callers": args.callers},
               "speedup": round(best_loop / best_batch, 2),
               "batch_equals_single_calls": batch == single}
        line["sets"].append(rec)
        print(json.dumps(rec), file=sys.stderr, flush=True)
    lib.zmx_set_kernel_timing(1)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
