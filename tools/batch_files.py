"""Many small files: one zmx_compress_batch call against the 16-caller ZopfliCompress loop, in the same process.

The two sets of bench.py's `small_files` line — 1000 x 64 KiB and 200 x 1 MB, classes T and X alternating (seeds 1000 ...),
the reference's default options with numiterations = 15, gzip.  For each set: MB/s of one batch call (after a warm-up batch),
MB/s of 16 caller threads each calling ZopfliCompress on one file at a time (after a warm-up round), and whether every
batch output equals the single call's.  Prints one JSON line.

usage: python tools/batch_files.py [--sets 1000x65536,200x1000000] [--callers 16] [--repeat 2]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="1000x65536,200x1000000")
    ap.add_argument("--callers", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=2, help="timed repetitions of each way (the best counts)")
    args = ap.parse_args()
    lib = api.library()
    lib.zmx_set_kernel_timing(0)     # (as any caller that does not ask for the phase times)
    opts = ZopfliOptions(15, 1, 15)
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
