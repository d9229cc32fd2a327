#!/usr/bin/env python3
"""Polyphase reordering at scale: the seeded hexaploid block of tests/reorder_cases.large_problem() (--positions, default 20 000; three reads
per position) through whatshap_amd.reorder.link_likelihoods_batch.  --warmup calls, then --steps timed calls; prints one JSON line and
appends it to profiles/reorder/bench.jsonl (--out): the whole call (wall, from the numpy arrays to the result arrays), the library's split
(host: validation, matrix rows, windows, read lists; upload / kernel / download from HIP events), median and min - max over the steps.
Measured against the debug library's host twin on one thread on the same host (--no-host skips it), which must return the same bits.
The reference's own Python loop on this block: tests/golden/make_reorder_golden.py --baseline N (profiles/reorder/cpu_baseline.md).
Not a bench.py entry.

    python scripts/gpu_reorder_bench.py [--positions 20000] [--steps 5] [--warmup 1] [--no-host] [--out profiles/reorder/bench.jsonl]
"""
import argparse
import collections
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import reorder_cases as rc  # noqa: E402
from whatshap_amd import reorder  # noqa: E402


def spread(values):
    return {"median": round(statistics.median(values), 3), "min": round(min(values), 3), "max": round(max(values), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=20_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reorder", "bench.jsonl"))
    a = ap.parse_args()
    case = rc.large_problem(a.positions)
    problem = rc.problem(case)
    for _ in range(a.warmup):   # code objects, the pools' blocks
        reorder.link_likelihoods_batch([problem])
    walls, stats, got = [], [], None
    for _ in range(a.steps):
        st = []
        t0 = time.perf_counter()
        got = reorder.link_likelihoods_batch([problem], stats=st)[0]
        walls.append((time.perf_counter() - t0) * 1e3)
        stats.append(st[0])
    s0 = stats[0]
    sizes = collections.Counter(len(b[1]) for b in case["breakpoints"])
    out = {
        "workload": "hexaploid_block", "positions": case["n_pos"], "reads": len(case["reads"]), "ploidy": case["ploidy"], "steps": a.steps, "warmup": a.warmup,
        **{k: int(s0[k]) for k in ("n_breakpoints", "n_reads_visited", "n_permutations", "n_window_positions", "launches")},
        "breakpoints_by_affected": {str(k): sizes[k] for k in sorted(sizes)},
        "whole_call_ms": spread(walls),
        "library": {k: spread([s[k] for s in stats]) for k in ("host_ms", "upload_ms", "kernel_ms", "download_ms", "total_ms")},
    }
    if not a.no_host:
        st = []
        t0 = time.perf_counter()
        twin = reorder.link_likelihoods_batch([problem], host=True, stats=st)[0]
        host_s = time.perf_counter() - t0
        out["host_twin_one_thread"] = {"whole_call_ms": round(host_s * 1e3, 3), "after_preparation_ms": round(st[0]["total_ms"] - st[0]["host_ms"], 3),
                                       "identical_to_device": bool(np.array_equal(twin.llh_flat.view(np.uint64), got.llh_flat.view(np.uint64))
                                                                   and np.array_equal(twin.threads, got.threads) and np.array_equal(twin.haplotypes, got.haplotypes))}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
