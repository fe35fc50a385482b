"""Many small files: one zmx_compress_batch call against the 16-caller ZopfliCompress loop, in the same process.

The two sets of bench.py's `small_files` line — 1000 x 64 KiB and 200 x 1 MB, classes T and X alternating (seeds 1000 ...),
the reference's default options with numiterations = 15, gzip.  For each set: MB/s of one batch call (after a warm-up batch),
MB/s of 16 caller threads each calling ZopfliCompress on one file at a time (after a warm-up round), and whether every
batch output equals the single call's.  Prints one JSON line.

--device: the same sets as tensors in device memory, four ways in one process — one zmx_compress_device_batch call, the
16-caller loop of zmx_compress_device (all there was before the device batch), zmx_compress_batch of host copies, and
zmx_gather_device alone (HIP events) beside one hipMemcpyAsync of the same total and n hipMemcpyAsync calls, with
co-aligned sources and with sources 1 byte off.  The outputs of the three compressing ways are compared.

--device-out: the same sets compressed INTO device memory, four ways in one process, each warmed once and then timed
--repeat times (3 by default here; the best counts, max - min is the spread): zmx_compress_device_batch_to_device with a
destination of zmx_compress_bound bytes per input, zmx_compress_device_batch_packed, this build's
zmx_compress_device_batch and, with --parent-lib PATH, the parent commit's (tools/build_variant.py builds one from a
checkout of it).  The condition printed is that the new entry is not slower than the parent's zmx_compress_device_batch by
more than the parent's spread in this run.  Then the join alone: k_bitjoin_many in the call itself (HIP events, the set's
own plan) and, on a plan of the same destinations made from the streams — per stream a byte-aligned head, the body at a
bit shift, a byte-aligned tail — one k_bitjoin_many launch, one k_bitjoin over the same pieces rebased into a packed
arena, one hipMemcpyAsync of the same bytes (events), and n zmx_bitjoin_device calls (wall clock); and the wall time of a
join of 2 100 and of 70 000 destinations of 20 bytes (the C call alone).

usage: python tools/batch_files.py [--sets 1000x65536,200x1000000] [--callers 16] [--repeat 2] [--device]
       python tools/batch_files.py --device-out [--parent-lib PATH] [--align 1]
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


def _timed(repeat, fn):
    """(best seconds, spread seconds, last result) of `repeat` runs after one warm-up run."""
    fn()
    times, out = [], None
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return min(times), max(times) - min(times), out


def _join_plan(streams_arena, offsets, sizes, shifted, shifted_at):
    """A plan with the destinations of the set's streams: stream i from three pieces — its first 64 bytes and its last 8
    from the packed streams themselves (byte-aligned, as the literals are), the body from a copy that lies i % 31 + 1 bits
    off (as the bit writer's buffers do).  pieces: (src, src_bit, nbits, dst_bit within the stream)."""
    dests, pieces = [], []
    for i, (off, size) in enumerate(zip(offsets, sizes)):
        head, tail = min(64, size), min(8, max(size - 64, 0))
        body = size - head - tail
        mine = [(streams_arena + off, 0, 8 * head, 0)]
        if body:
            mine.append((shifted + shifted_at[i], i % 31 + 1 + 8 * head, 8 * body, 8 * head))
        if tail:
            mine.append((streams_arena + off + size - tail, 0, 8 * tail, 8 * (size - tail)))
        dests.append((len(pieces), len(mine)))
        pieces += mine
    return dests, pieces


def _join_rates(lib, hip, streams, repeat):
    """The join alone on the destinations of `streams` (the set's outputs, bytes objects)."""
    import ctypes

    import numpy as np
    import torch

    from zopfli_amd import Context
    lib.zmx_internal_bitjoin_ms.restype = ctypes.c_double
    sizes = [len(s) for s in streams]
    offsets, at = [], 0
    for n in sizes:
        offsets.append(at)
        at += n
    total = at
    packed = torch.frombuffer(bytearray(b"".join(streams)), dtype=torch.uint8).cuda()
    # the bodies' source: every stream shifted up by i % 31 + 1 bits, in a stretch of its own (8-byte aligned)
    shifted_at, parts, at = [], [], 0
    for i, s in enumerate(streams):
        shifted_at.append(at)
        v = int.from_bytes(s, "little") << (i % 31 + 1)
        parts.append(v.to_bytes((len(s) + 4 + 7) // 8 * 8, "little"))
        at += len(parts[-1])
    shifted = torch.frombuffer(bytearray(b"".join(parts)), dtype=torch.uint8).cuda()
    drange, pieces = _join_plan(packed.data_ptr(), offsets, sizes, shifted.data_ptr(), shifted_at)
    dst = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
    d = dst.data_ptr() + 16
    many = [(d + off, 8 * size, first, n) for off, size, (first, n) in zip(offsets, sizes, drange)]
    rebased = [(src, sb, nb, db + 8 * off) for off, (first, n) in zip(offsets, drange) for src, sb, nb, db in pieces[first:first + n]]
    ctx = Context(0, lib)
    lib.zmx_set_kernel_timing(1)
    torch.cuda.synchronize()
    reps = max(repeat, 3)
    out = {"destinations": len(sizes), "pieces": len(pieces), "bytes": total}
    try:
        def events(fn):
            best_ms, best_wall = None, None
            for _ in range(reps + 1):
                t0 = time.perf_counter()
                fn()
                wall = (time.perf_counter() - t0) * 1e3
                ms = lib.zmx_internal_bitjoin_ms()
                best_ms = ms if best_ms is None else min(best_ms, ms)
                best_wall = wall if best_wall is None else min(best_wall, wall)
            return best_ms, best_wall
        gbs = lambda ms: round(total / 1e9 / (ms / 1e3), 2) if ms else None   # noqa: E731
        ms, wall = events(lambda: ctx.bitjoin_many_device(many, pieces))
        equal = bool(torch.equal(dst[16:16 + total], packed)) and bool(torch.all(dst[:16] == 0xA5).item()) and \
            bool(torch.all(dst[16 + total:] == 0xA5).item())
        out["k_bitjoin_many"] = {"GB/s": gbs(ms), "ms": round(ms, 4), "call_wall_ms": round(wall, 3), "equals_the_streams": equal}
        dst.fill_(0xA5)
        torch.cuda.synchronize()
        ms, wall = events(lambda: ctx.bitjoin_device(rebased, 8 * total, d, total))
        out["k_bitjoin_packed"] = {"GB/s": gbs(ms), "ms": round(ms, 4), "call_wall_ms": round(wall, 3),
                                   "equals_the_streams": bool(torch.equal(dst[16:16 + total], packed))}
        hip.copies_ms(d, [(packed.data_ptr(), total)])
        one_ms = min(hip.copies_ms(d, [(packed.data_ptr(), total)]) for _ in range(reps))
        out["one_hipMemcpyAsync"] = {"GB/s": gbs(one_ms), "ms": round(one_ms, 4)}

        def loop():
            for off, size, (first, n) in zip(offsets, sizes, drange):
                ctx.bitjoin_device(pieces[first:first + n], 8 * size, d + off, size)
        lib.zmx_set_kernel_timing(0)
        loop()
        t0 = time.perf_counter()
        loop()
        wall = (time.perf_counter() - t0) * 1e3
        out["n_zmx_bitjoin_device_calls"] = {"wall_ms": round(wall, 2), "ms_per_call": round(wall / len(sizes), 4), "GB/s": gbs(wall)}
        # many tiny destinations: 20 bytes each, back to back, each one piece at a bit shift
        for count in (2100, 70000):
            src = torch.frombuffer(bytearray(np.random.default_rng(count).integers(0, 256, 24 * count + 8, dtype=np.uint8).tobytes()),
                                   dtype=torch.uint8).cuda()
            tiny = torch.full((20 * count + 32,), 0xA5, dtype=torch.uint8, device="cuda:0")
            td = [(tiny.data_ptr() + 5 + 20 * i, 160, i, 1) for i in range(count)]
            tp = [(src.data_ptr() + 24 * i, i % 31 + 1, 160, 0) for i in range(count)]
            torch.cuda.synchronize()
            ctx.bitjoin_many_device(td, tp)
            # (the C call alone: the tables as the arrays it takes, made once)
            darr = (ctypes.c_uint64 * (4 * count))(*[v for t in td for v in t])
            parr = (ctypes.c_uint64 * (4 * count))(*[v for t in tp for v in t])
            fn = lib.zmx_bitjoin_many_device
            walls = []
            for _ in range(reps):
                t0 = time.perf_counter()
                rc = fn(ctx.handle, count, ctypes.cast(darr, ctypes.c_void_p), None, count, ctypes.cast(parr, ctypes.c_void_p))
                walls.append((time.perf_counter() - t0) * 1e3)
                assert rc == 0
            host = src.cpu().numpy()
            got = tiny.cpu().numpy()
            ok = bool(np.all(got[:5] == 0xA5)) and bool(np.all(got[5 + 20 * count:] == 0xA5))
            for i in (0, 1, count // 2, count - 1):
                v = (int.from_bytes(host[24 * i:24 * i + 24].tobytes(), "little") >> (i % 31 + 1)) & ((1 << 160) - 1)
                ok = ok and got[5 + 20 * i:25 + 20 * i].tobytes() == v.to_bytes(20, "little")
            out["tiny_%d" % count] = {"call_wall_ms": round(min(walls), 3), "right": ok}
    finally:
        lib.zmx_set_kernel_timing(0)
        ctx.close()
    return out


def device_out_main(args, lib, opts):
    import ctypes

    import torch
    hip = _Hip()
    parent = api.library(os.path.abspath(args.parent_lib)) if args.parent_lib else None
    lib.zmx_internal_bitjoin_ms.restype = ctypes.c_double
    line = {"metric": "many inputs in device memory compressed INTO device memory: zmx_compress_device_batch_to_device and "
                      "zmx_compress_device_batch_packed vs zmx_compress_device_batch of this build and of the parent commit",
            "options": "blocksplitting=1, blocksplittingmax=15, numiterations=15, gzip", "repeat": args.repeat, "sets": []}
    for spec in args.sets.split(","):
        count, size = (int(x) for x in spec.split("x"))
        files = [generate("TX"[i & 1], size, seed=1000 + i) for i in range(count)]
        tensors = [torch.frombuffer(bytearray(f), dtype=torch.uint8).cuda() for f in files]
        bound = api.compress_bound(size, api.FORMAT_GZIP, lib=lib)
        dsts = [torch.empty(bound, dtype=torch.uint8, device="cuda") for _ in range(count)]
        arena = torch.empty(api.compress_batch_bound([size] * count, api.FORMAT_GZIP, args.align, lib=lib), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        total = count * size / MB
        rec = {"files": count, "bytes_each": size, "classes": "T and X alternating, seeds 1000 ...", "ways": {}}

        def way(name, fn):
            best, spread, out = _timed(args.repeat, fn)
            rec["ways"][name] = {"value": round(total / best, 3), "unit": "MB/s", "ms": round(best * 1e3, 1), "spread_ms": round(spread * 1e3, 1)}
            return best, spread, out
        new, _, sizes = way("device_batch_to_device", lambda: api.compress_device_batch_out(tensors, dsts, api.FORMAT_GZIP, opts, lib=lib))
        rec["output_traffic"] = api.last_output_traffic(lib)
        rec["input_traffic"] = api.last_input_traffic(lib)
        _, _, (offsets, psizes) = way("device_batch_packed", lambda: api.compress_device_batch_packed(tensors, arena, args.align, api.FORMAT_GZIP, opts, lib=lib))
        _, _, host = way("device_batch", lambda: api.compress_device_batch(tensors, api.FORMAT_GZIP, opts, lib=lib))
        got_arena = arena.cpu().numpy()
        rec["outputs_equal"] = sizes == [len(h) for h in host] and psizes == sizes and \
            all(d[:n].cpu().numpy().tobytes() == h for d, n, h in zip(dsts, sizes, host)) and \
            all(got_arena[o:o + n].tobytes() == h for o, n, h in zip(offsets, psizes, host))
        rec["stream_bytes"] = sum(sizes)
        if parent is not None:
            pbest, pspread, pout = way("device_batch_parent", lambda: api.compress_device_batch(tensors, api.FORMAT_GZIP, opts, lib=parent))
            rec["outputs_equal"] = rec["outputs_equal"] and pout == host
            rec["not_slower_than_parent_by_more_than_its_spread"] = bool(new <= pbest + pspread)
            rec["condition"] = "%.1f ms against %.1f + %.1f ms" % (new * 1e3, pbest * 1e3, pspread * 1e3)
        lib.zmx_set_kernel_timing(1)
        api.compress_device_batch_out(tensors, dsts, api.FORMAT_GZIP, opts, lib=lib)
        rec["k_bitjoin_many_in_the_call_ms"] = round(lib.zmx_internal_bitjoin_ms(), 4)
        lib.zmx_set_kernel_timing(0)
        del tensors, dsts, arena
        rec["join"] = _join_rates(lib, hip, host, args.repeat)
        line["sets"].append(rec)
        print(json.dumps(rec), file=sys.stderr, flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="1000x65536,200x1000000")
    ap.add_argument("--callers", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=None, help="timed repetitions of each way (the best counts): 2, --device-out 3")
    ap.add_argument("--device", action="store_true", help="the sets as tensors in device memory (see above)")
    ap.add_argument("--device-out", action="store_true", help="the sets compressed into device memory (see above)")
    ap.add_argument("--parent-lib", default=None, help="--device-out: libzopfli_amd.so of the parent commit")
    ap.add_argument("--align", type=int, default=1, help="--device-out: the packed form's alignment")
    args = ap.parse_args()
    if args.repeat is None:
        args.repeat = 3 if args.device_out else 2
    if args.device or args.device_out:
        import torch  # noqa: F401  (before the library: both then share torch's HIP runtime, and its tensors are device memory to the library)
    lib = api.library()
    lib.zmx_set_kernel_timing(0)     # (as any caller that does not ask for the phase times)
    opts = ZopfliOptions(15, 1, 15)
    if args.device_out:
        line = device_out_main(args, lib, opts)
        lib.zmx_set_kernel_timing(1)
        print(json.dumps(line), flush=True)
        return
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
