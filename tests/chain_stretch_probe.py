"""Run by tests/test_gpu_chain_stretch.py in a subprocess (the task geometry of the chain kernels is read from the
environment once per process): one case, named by STRETCH_PROBE_CASE, through three chained squeeze runs against the
CPU oracle (length_array, stores, histograms, symbol counts), then one JSON line: how the chain's tasks fared
(zmx_last_seg_stats), the non-empty blocks of the case, and a digest of everything the runs produced."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import oracle_lib as ol  # noqa: E402
from zopfli_amd import Context, api, generate  # noqa: E402

# Block sizes for ZOPFLI_AMD_SEG_L=256, ZOPFLI_AMD_SEG_HEAD=0: the head is 256 positions, a block of B positions has
# 1 task below 512 and 1 + (B - 256) / 256 from there on.
EDGE_STRETCH = 16
EDGE_TASKS = [1, 2, 4, 5, 6, 0, 1, EDGE_STRETCH + 1]              # (0: the empty block; the 20-byte block has one task)
EDGE_SIZES = [300, 600, 1100, 1400, 1600, 0, 20, 256 * (EDGE_STRETCH + 1) + 100]


def tasks_of(size, seg_l=256):
    return 0 if size == 0 else 1 if size < 2 * seg_l else 1 + (size - seg_l) // seg_l


def blocks_of(sizes):
    out, at = [], 0
    for n in sizes:
        out.append((at, at + n))
        at += n
    return out


def mixed_data(n=150000, seed=11):
    """Text pieces and long-run (class Z) pieces glued, seeded: text-kind and run-kind tasks interleave in the block."""
    rng = np.random.default_rng(seed)
    text, runs = generate("T", n), generate("Z", n)
    parts, at, k = [], 0, 0
    while at < n:
        m = min(int(rng.integers(3000, 14000)), n - at)
        parts.append((text if k % 2 == 0 else runs)[at:at + m])
        at += m
        k += 1
    return b"".join(parts)


def case(name):
    """(data, blocks)"""
    if name == "edges":
        assert [tasks_of(n) for n in EDGE_SIZES] == EDGE_TASKS
        return generate("T", sum(EDGE_SIZES)), blocks_of(EDGE_SIZES)
    if name == "binade":
        return generate("T", 65536), [(0, 65536)]
    if name == "mixed":
        return mixed_data(), [(0, 150000)]
    if name == "redo200k":
        return generate("T", 200000), [(0, 120000), (120000, 200000)]
    if name == "redo40k":
        return generate("T", 40000), [(0, 40000)]
    raise SystemExit(f"unknown case {name}")


def squeeze_runs_against_oracle(t, data, blocks):
    """Three chained squeeze runs on the tables `t` of `blocks` of `data`, each held to the CPU oracle (length_array,
    stores, histograms, symbol counts; the first mismatch is printed and ends the process with status 1).  -> the
    digest of everything the runs produced."""
    nb = len(blocks)
    nsym, hist = t.greedy(0)
    tables = [ol.OracleTable(data, s, e) for (s, e) in blocks]
    digest = hashlib.sha256()
    for it in range(3):
        cost = np.zeros((nb, 320))
        mincost = np.zeros(nb)
        for b in range(nb):
            ll, d = ol.entropy_costs(hist[b])
            cost[b, :288], cost[b, 288:] = ll, d
            mincost[b] = ol.model_min_cost(ll, d)
        nsym, hist = t.squeeze_run(cost, mincost, np.full(nb, it & 1, dtype=np.int32))
        for b, (s, e) in enumerate(blocks):
            la, oll, odd = tables[b].squeeze_run(cost[b, :288], cost[b, 288:], mincost[b])
            what = f"iter {it} block {b}"
            if e > s:
                gla = t.length_array(b)
                if not np.array_equal(gla[1:], la[1:]):
                    bad = int(np.nonzero(gla[1:] != la[1:])[0][0]) + 1
                    print(f"MISMATCH {what}: length_array differs first at {bad}", flush=True)
                    sys.exit(1)
                digest.update(np.ascontiguousarray(gla[1:]).tobytes())
            gll, gdd = t.store(b, it & 1, nsym[b])
            if nsym[b] != len(oll):
                print(f"MISMATCH {what}: nsym {nsym[b]} vs {len(oll)}", flush=True)
                sys.exit(1)
            if not (np.array_equal(gll, oll) and np.array_equal(gdd, odd)):
                print(f"MISMATCH {what}: store", flush=True)
                sys.exit(1)
            if not np.array_equal(hist[b], ol.histogram(oll, odd)):
                print(f"MISMATCH {what}: histogram", flush=True)
                sys.exit(1)
            digest.update(np.ascontiguousarray(gll).tobytes() + np.ascontiguousarray(gdd).tobytes())
            digest.update(np.ascontiguousarray(hist[b]).tobytes())
    return digest.hexdigest()


def main():
    data, blocks = case(os.environ["STRETCH_PROBE_CASE"])
    lib = api.library()
    ctx = Context(0, lib)
    ctx.set_input(data)
    t = ctx.build_tables(blocks)
    digest = squeeze_runs_against_oracle(t, data, blocks)
    t.free()
    ctx.close()
    st = api.last_seg_stats(lib)
    st["blocks"] = sum(1 for (s, e) in blocks if e > s)
    st["digest"] = digest
    print(json.dumps(st), flush=True)


if __name__ == "__main__":
    main()
