#!/usr/bin/env python3
"""Comparing polyploid phasings at scale, through whatshap_amd.compare.compare_blocks: --blocks (default 2 000) seeded hexaploid blocks of
--positions (default 500) positions in one call, and one hexaploid block of --long-positions (default 100 000).  --warmup calls, then --steps
timed calls of each; prints one JSON line per workload and appends it to profiles/compare/bench.jsonl (--out): the whole call (wall, from
the numpy arrays to the PhasingErrors), the library's split (host: validation and matching positions; upload / kernel / download from HIP
events), median and min - max over the steps.
Measured against the debug library's host twin on one thread on the same host, which must return the same results: on the first
--host-blocks blocks and on the first --host-long-positions positions of the long block (a whole workload takes the twin many minutes;
the figure scales with the block count, and with the length).  --no-host skips it.
The reference's own compare_block: tests/golden/make_compare_golden.py --baseline N (profiles/compare/cpu_baseline.md).
Not a bench.py entry.

    python scripts/gpu_compare_bench.py [--blocks 2000] [--positions 500] [--long-positions 100000] [--steps 3] [--warmup 1] [--no-host]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import compare_cases as cc  # noqa: E402
from whatshap_amd import compare  # noqa: E402


def spread(values):
    return {"median": round(statistics.median(values), 3), "min": round(min(values), 3), "max": round(max(values), 3)}


def timed(blocks, steps, warmup):
    t0 = time.perf_counter()
    for _ in range(warmup):   # code objects, the pools' blocks
        compare.compare_blocks(blocks)
    warm_ms = (time.perf_counter() - t0) * 1e3
    walls, stats, got = [], [], None
    for _ in range(steps):
        st = []
        t0 = time.perf_counter()
        got = compare.compare_blocks(blocks, stats=st)
        walls.append((time.perf_counter() - t0) * 1e3)
        stats.append(st[0])
    out = {**{k: int(stats[0][k]) for k in ("n_jobs", "n_positions", "n_visited", "launches")}, "warmup_calls_ms": round(warm_ms, 3), "whole_call_ms": spread(walls),
           "library": {k: spread([s[k] for s in stats]) for k in ("host_ms", "upload_ms", "kernel_ms", "download_ms", "total_ms")}}
    return out, got


def host_twin(blocks, got):
    st = []
    t0 = time.perf_counter()
    twin = compare.compare_blocks(blocks, host=True, stats=st)
    return {"blocks": len(blocks), "positions_per_block": len(blocks[0][0]), "whole_call_ms": round((time.perf_counter() - t0) * 1e3, 3),
            "after_preparation_ms": round(st[0]["total_ms"] - st[0]["host_ms"], 3), "identical_to_device": [repr(t) for t in twin] == [repr(g) for g in got]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=2000)
    ap.add_argument("--positions", type=int, default=500)
    ap.add_argument("--long-positions", type=int, default=100_000)
    ap.add_argument("--host-blocks", type=int, default=4)
    ap.add_argument("--host-long-positions", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compare", "bench.jsonl"))
    a = ap.parse_args()
    lines = []
    if a.blocks:
        blocks = [cc.bench_block(seed, n_pos=a.positions) for seed in range(a.blocks)]
        out, got = timed(blocks, a.steps, a.warmup)
        out = {"workload": "hexaploid_blocks", "blocks": a.blocks, "positions": a.positions, "ploidy": 6, "steps": a.steps, "warmup": a.warmup, **out}
        if not a.no_host:
            n = min(a.host_blocks, a.blocks)
            out["host_twin_one_thread"] = host_twin(blocks[:n], got[:n])
        lines.append(out)
    if a.long_positions:
        p0, p1 = cc.bench_block(12345, n_pos=a.long_positions)
        out, got = timed([(p0, p1)], a.steps, a.warmup)
        out = {"workload": "one_long_hexaploid_block", "positions": a.long_positions, "ploidy": 6, "steps": a.steps, "warmup": a.warmup, **out,
               "result": repr(got[0])}
        if not a.no_host:
            n = min(a.host_long_positions, a.long_positions)
            head = [(p0[:n], p1[:n])]
            out["host_twin_one_thread"] = host_twin(head, compare.compare_blocks(head))
        lines.append(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for out in lines:
        line = json.dumps(out)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
