"""A PNG left in device memory: the two checksum kernels alone, and the to-device PNG entries against the host-output ones.

(a) k_checksum_pieces and k_checksum_finish alone, by HIP events (zmx_internal_checksum_device_ms), on the IDAT of the
    photograph-like 4096 x 4096 RGBA8 image's file (one range of about 26 MB, where the file lies: 37 bytes behind the
    destination's start) and on the IDATs of the 1 000 files of the 64 x 64 icons in their packed arena (1 000 ranges of
    1 - 3 KB at whatever alignment the packing gave them).  Beside them, by the wall clock: the whole zmx_checksum_device
    call, and zmx_checksum / zmx_checksums (k_checksum / k_checksums, finished on the host) on a resident copy of the same
    bytes; and one hipMemcpyAsync device to device of the bytes (events) as the yardstick.  GB/s from the bytes read once.
(b) The calls, wall clock: zmx_png_encode_device_to_device of the 4096 x 4096 image (strategy e, numiterations 5) against
    zmx_png_encode_device, and zmx_png_encode_device_batch_packed of the 1 000 icons (numiterations 15) against
    zmx_png_encode_device_batch — of this build and, with --parent-lib, of the parent commit's library loaded in the
    same process (tools/build_variant.py builds one from a checkout of it).
    Condition: the new entry is not slower than the parent's host-output entry by more than the sum of the two spreads.
A process per table, the ways alternating after a warm-up of each, best of --repeat and the spread (max - min).

usage: python tools/png_device_output.py [--repeat 5] [--size 4096] [--icons 1000] [--parent-lib PATH]
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

PREFIX, TRAILER = 41, 16   # the file around the IDAT's payload (colour types 0, 2, 4, 6: no PLTE, no tRNS)


def _files(lib, args):
    """(big image, its file in `dst`, its size), (icons, their arena, offsets, sizes): made once per process."""
    import torch

    from zopfli_amd import ZopfliOptions, api
    big = torch.from_numpy(_image(args.size)).cuda()
    dst = torch.empty(api.png_bound(args.size, args.size, 6, 8, lib=lib) + 3, dtype=torch.uint8, device="cuda")
    icons = [torch.from_numpy(_image(64, 100 + i)).cuda() for i in range(args.icons)]
    arena = torch.empty(api.png_batch_bound(icons, 1, lib=lib), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    size = api.png_encode_device_out(big, dst, "e", ZopfliOptions(5), lib=lib)
    offs, sizes = api.png_encode_device_batch_packed(icons, arena, 1, "e", ZopfliOptions(15), lib=lib)
    return (big, dst, size), (icons, arena, offs, sizes)


def _kernels(args):
    import torch

    from batch_files import _Hip
    from zopfli_amd import Context, api
    lib = api.library()
    lib.zmx_set_kernel_timing(0)
    (_, dst, size), (_, arena, offs, sizes) = _files(lib, args)
    ms2 = (ctypes.c_double * 2)()
    lib.zmx_internal_checksum_device_ms.argtypes = [ctypes.POINTER(ctypes.c_double)]
    lib.zmx_internal_checksum_device_ms.restype = None
    hip = _Hip()
    ctx, resident = Context(0, lib), Context(0, lib)
    out = {}
    inputs = {
        f"one IDAT of the {args.size} x {args.size} file": [(dst.data_ptr() + PREFIX - 4, 4 + size - PREFIX - TRAILER)],
        f"the IDATs of {args.icons} icon files": [(arena.data_ptr() + o + PREFIX - 4, 4 + s - PREFIX - TRAILER) for o, s in zip(offs, sizes)],
    }
    try:
        for name, ranges in inputs.items():
            total = sum(n for _, n in ranges)
            # a resident, aligned copy of the same bytes end to end for the parent's kernels
            copy = torch.empty(total, dtype=torch.uint8, device="cuda")
            spare = torch.empty(total, dtype=torch.uint8, device="cuda")
            hip.copies_ms(copy.data_ptr(), ranges)
            resident.set_input_device(copy.data_ptr(), total)
            spans, at = [], 0
            for _, n in ranges:
                spans.append((at, at + n))
                at += n
            got = {}
            pieces, finish = [], []

            def device():
                got["device"] = ctx.checksum_device(0, ranges)

            def device_timed():
                lib.zmx_set_kernel_timing(1)
                ctx.checksum_device(0, ranges)
                lib.zmx_internal_checksum_device_ms(ms2)
                lib.zmx_set_kernel_timing(0)
                pieces.append(ms2[0])
                finish.append(ms2[1])

            def parent():
                got["resident"] = resident.checksums(0, spans) if len(spans) > 1 else [resident.checksum(0, 0, total)]

            copies = []

            def memcpy():
                copies.append(hip.copies_ms(spare.data_ptr(), [(copy.data_ptr(), total)]))

            wall = _alternate({"zmx_checksum_device, the call (wall)": device, "events": device_timed,
                               "k_checksum" + ("s" if len(spans) > 1 else "") + " + host finish on a resident copy, the call (wall)": parent,
                               "memcpy": memcpy}, args.repeat)
            rec = {"ranges": len(ranges), "bytes": total, "equal": got["device"] == got["resident"]}
            rec["k_checksum_pieces (events)"] = _stats(pieces[1:])
            rec["k_checksum_finish (events)"] = _stats(finish[1:])
            rec["both kernels (events)"] = _stats([a + b for a, b in zip(pieces[1:], finish[1:])])
            for key in wall:
                if key not in ("events", "memcpy"):
                    rec[key] = _stats(wall[key])
            rec["one hipMemcpyAsync of the bytes (events)"] = _stats(copies[1:])
            for key, s in rec.items():
                if isinstance(s, dict):
                    s["GB/s"] = round(total / 1e9 / (s["best_ms"] / 1e3), 1) if s["best_ms"] > 0 else None
            out[name] = rec
    finally:
        ctx.close()
        resident.close()
    return out


def _calls(args):
    import torch

    from zopfli_amd import ZopfliOptions, api
    lib = api.library()
    lib.zmx_set_kernel_timing(0)
    parent = None
    if args.parent_lib:
        parent = api.bind(ctypes.CDLL(os.path.abspath(args.parent_lib)))
        parent.zmx_set_kernel_timing(0)
    (big, dst, _), (icons, arena, _, _) = _files(lib, args)
    got = {}
    out = {}

    big_ways = {
        "zmx_png_encode_device_to_device": lambda: got.__setitem__("big_out", api.png_encode_device_out(big, dst, "e", ZopfliOptions(5), lib=lib)),
        "zmx_png_encode_device": lambda: got.__setitem__("big", api.png_encode_device(big, "e", ZopfliOptions(5), lib=lib)),
    }
    icon_ways = {
        "zmx_png_encode_device_batch_packed": lambda: got.__setitem__("icons_out", api.png_encode_device_batch_packed(icons, arena, 1, "e", ZopfliOptions(15), lib=lib)),
        "zmx_png_encode_device_batch": lambda: got.__setitem__("icons", api.png_encode_device_batch(icons, "e", ZopfliOptions(15), lib=lib)),
    }
    if parent is not None:
        big_ways["zmx_png_encode_device, parent commit"] = lambda: api.png_encode_device(big, "e", ZopfliOptions(5), lib=parent)
        icon_ways["zmx_png_encode_device_batch, parent commit"] = lambda: api.png_encode_device_batch(icons, "e", ZopfliOptions(15), lib=parent)
    for table, ways in ((f"{args.size} x {args.size} RGBA8, strategy e, numiterations 5", big_ways),
                        (f"{args.icons} x 64 x 64 RGBA8, strategy e, numiterations 15", icon_ways)):
        rec = {name: _stats(v) for name, v in _alternate(ways, args.repeat).items()}
        names = list(ways)
        new, old = rec[names[0]], rec[names[-1]]
        rec["against"] = names[-1]
        rec["difference_ms"] = round(new["best_ms"] - old["best_ms"], 2)
        rec["allowed_ms"] = round(new["spread_ms"] + old["spread_ms"], 2)
        rec["holds"] = rec["difference_ms"] <= rec["allowed_ms"]
        out[table] = rec
    torch.cuda.synchronize()
    size = got["big_out"]
    out["files_equal"] = {"big": dst[:size].cpu().numpy().tobytes() == got["big"],
                          "icons": [arena[o:o + s].cpu().numpy().tobytes() for o, s in zip(*got["icons_out"])] == got["icons"]}
    out["output_traffic_of_the_packed_batch"] = None
    api.png_encode_device_batch_packed(icons, arena, 1, "e", ZopfliOptions(15), lib=lib)
    out["output_traffic_of_the_packed_batch"] = api.last_output_traffic(lib)
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
    print(f"  {name:<76}{s['best_ms']:>12.4f}{s['spread_ms']:>11.4f}{extra}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--icons", type=int, default=1000)
    ap.add_argument("--parent-lib", default=None, help="libzopfli_amd.so of the parent commit")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(TABLES[args.child](args)), flush=True)
        return
    results = {}
    head = f"  {'':<76}{'best ms':>12}{'spread ms':>11}"
    results["kernels"] = kern = _child("kernels", args)
    print(f"(a) the checksum kernels alone, CRC-32, best of {args.repeat} after a warm-up")
    for name, rec in kern.items():
        print(f"\n {name}: {rec['ranges']} range(s), {rec['bytes']} bytes; values equal the resident kernels': {rec['equal']}")
        print(head + "       GB/s")
        for key, s in rec.items():
            if isinstance(s, dict):
                _line(key, s, f"{s['GB/s']:>11.1f}" if s.get("GB/s") is not None else "")
    results["calls"] = calls = _child("calls", args)
    print(f"\n(b) the calls (wall, one process, ways alternating), best of {args.repeat} after a warm-up")
    for table, rec in calls.items():
        if not isinstance(rec, dict) or "against" not in rec:
            continue
        print(f"\n {table}")
        print(head)
        for key, s in rec.items():
            if isinstance(s, dict):
                _line(key, s)
        print(f"  the to-device entry - {rec['against']} = {rec['difference_ms']} ms; allowed: both spreads = {rec['allowed_ms']} ms: "
              f"{'holds' if rec['holds'] else 'DOES NOT HOLD'}")
    print(f"\n  the files in device memory equal the host-output entries': {calls['files_equal']}")
    print(f"  zmx_last_output_traffic of the packed batch [down, up, device blocks, host blocks]: {calls['output_traffic_of_the_packed_batch']}")
    print()
    print(json.dumps({"repeat": args.repeat, "size": args.size, "icons": args.icons, "parent_lib": bool(args.parent_lib), "results": results}))


if __name__ == "__main__":
    main()
