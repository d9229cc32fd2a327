#!/usr/bin/env python3
"""Polyphase threading inputs at scale: the seeded hexaploid chromosome of tests/polythread_cases.py (bench_arrays: --positions positions,
default 500 000, reads of 30 consecutive positions at --coverage 40, clusters of about 2 000 positions per haplotype) through
whatshap_amd.polythread.threading_inputs_batch, and a batch of --blocks small blocks (default 2 000) in one call.  One warm-up call, then
--repeat timed calls each; prints one JSON line per workload and appends it to profiles/polythread/bench.jsonl (--out): reads, entries,
positions and rows of the problem, the whole call (wall, from the numpy arrays to the result arrays), the library's split (host:
validation, matrix rows, reads to (cluster, rank); upload / kernel / download from HIP events; fill: gap filling and assembly on the
host), median and min - max over the repeats, entries/s of the kernels and of the whole call.  And the debug library's host twin on one
thread, which must return the same bytes (--no-host skips it).  Not a bench.py entry.

    python scripts/gpu_polythread_bench.py [--positions 500000] [--coverage 40] [--blocks 2000] [--repeat 5] [--no-host] [--out profiles/polythread/bench.jsonl]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import polythread_cases as pc  # noqa: E402
from gpu_haplotag_bench import spread  # noqa: E402
from whatshap_amd import polythread as pt  # noqa: E402

COUNTS = ("n_reads", "n_positions", "n_entries", "n_counted", "n_rows", "n_selected", "n_readded", "n_emptied", "positions_class_a", "positions_class_b",
          "positions_class_c")


def measure(workload, problems, repeat, host, out_path, extra):
    pt.threading_inputs_batch(problems)   # warm-up: code objects, the pools' blocks
    walls, stats = [], []
    got = None
    for _ in range(repeat):
        st = []
        t0 = time.perf_counter()
        got = pt.threading_inputs_batch(problems, stats=st)
        walls.append((time.perf_counter() - t0) * 1e3)
        stats.append(st)
    n_entries = sum(s["n_entries"] for s in stats[0])
    kernel = spread([st[0]["kernel_ms"] for st in stats])
    out = {
        "workload": workload, "problems": len(problems), "repeat": repeat, **extra,
        **{k[2:] if k.startswith("n_") else k: int(sum(s[k] for s in stats[0])) for k in COUNTS},
        "launches": int(stats[0][0]["launches"]),
        "whole_call_ms": spread(walls),
        "library": {k: spread([st[0][k] for st in stats]) for k in ("host_ms", "upload_ms", "kernel_ms", "download_ms", "fill_ms", "total_ms")},
        "entries_per_s_kernel": n_entries / (kernel["median"] / 1e3),
        "entries_per_s_whole_call": n_entries / (statistics.median(walls) / 1e3),
    }
    if host:
        t0 = time.perf_counter()
        twin = pt.threading_inputs_batch(problems, host=True)
        host_s = time.perf_counter() - t0
        s = twin[0].stats
        out["host_twin_one_thread"] = {"whole_call_s": round(host_s, 3), "rows_and_selection_s": round((s["total_ms"] - s["host_ms"] - s["fill_ms"]) / 1e3, 3),
                                       "identical_to_device": bool(all(a.tobytes() == b.tobytes() for a, b in zip(twin, got)))}
    line = json.dumps(out)
    print(line, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=500_000)
    ap.add_argument("--coverage", type=int, default=40)
    ap.add_argument("--blocks", type=int, default=2000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polythread", "bench.jsonl"))
    a = ap.parse_args()
    if a.positions:
        chromosome = pc.problem_of_arrays(pc.bench_arrays(a.positions, a.coverage), pc.BENCH["ploidy"], pc.BENCH["max_gap"])
        measure("hexaploid_chromosome", [chromosome], a.repeat, not a.no_host, a.out, {"ploidy": pc.BENCH["ploidy"], "coverage": a.coverage})
    if a.blocks:
        blocks = [pc.problem_of_arrays(arrays, ploidy, gap) for arrays, ploidy, gap in pc.small_blocks(a.blocks)]
        measure("small_blocks", blocks, a.repeat, not a.no_host, a.out, {})


if __name__ == "__main__":
    main()
