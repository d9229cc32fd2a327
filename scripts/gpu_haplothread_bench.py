#!/usr/bin/env python3
"""The polyphase threading DP at scale: seeded problems of tests/haplothread_cases.py (bench_problem: ploidy + 2 clusters listed at every
position, depths wandering around levels of 5 .. 80, costs 12 / 3, max_cluster_gap 10) through whatshap_amd.polythread.thread_batch.
Workloads: --sections sections (default 2 000) of 500 positions in one call, and one section of --positions positions (default
100 000), hexaploid and tetraploid.  One warm-up call, then --repeat timed calls each; prints one JSON line per workload and appends it
to profiles/haplothread/bench.jsonl (--out): positions, tuples and surviving entries, the whole call (wall, from the numpy arrays to
the result arrays), the library's split (host: validation, smoothed coverages, log terms; upload / kernel / download from HIP events),
median and min - max over the repeats, the launch count, and the debug library's host twin on one thread, which must return the same
bytes (--no-host skips it).  A single long section is one workgroup on dependent columns.  Not a bench.py entry.

    python scripts/gpu_haplothread_bench.py [--sections 2000] [--positions 100000] [--repeat 5] [--no-host] [--out profiles/haplothread/bench.jsonl]
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

import haplothread_cases as hc  # noqa: E402
from gpu_haplotag_bench import spread  # noqa: E402
from whatshap_amd import polythread as pt  # noqa: E402


def problems_of(ploidy, n_sections, n_pos):
    return [pt.ThreaderProblem(*hc.bench_problem(ploidy, n_pos, seed=s), ploidy, 12.0, 3.0, 10) for s in range(n_sections)]


def measure(workload, ploidy, problems, repeat, host, out_path):
    pt.thread_batch(problems)   # warm-up: code objects, the pools' blocks
    walls, stats = [], []
    got = None
    for _ in range(repeat):
        t0 = time.perf_counter()
        got = pt.thread_batch(problems)
        walls.append((time.perf_counter() - t0) * 1e3)
        stats.append(got[0].stats)
    n_pos = sum(r.stats["n_positions"] for r in got)
    kernel = spread([s["kernel_ms"] for s in stats])
    out = {
        "workload": workload, "ploidy": ploidy, "problems": len(problems), "repeat": repeat, "positions": int(n_pos),
        "tuples": int(sum(r.stats["n_tuples"] for r in got)), "entries": int(sum(r.stats["n_entries"] for r in got)),
        "ambiguous_sections": int(sum(int(r.ambiguous.any()) for r in got)), "launches": int(stats[0]["launches"]),
        "whole_call_ms": spread(walls),
        "library": {k: spread([s[k] for s in stats]) for k in ("host_ms", "upload_ms", "kernel_ms", "download_ms", "total_ms")},
        "positions_per_s_kernel": n_pos / (kernel["median"] / 1e3),
        "positions_per_s_whole_call": n_pos / (statistics.median(walls) / 1e3),
    }
    if host:
        t0 = time.perf_counter()
        twin = pt.thread_batch(problems, host=True)
        host_s = time.perf_counter() - t0
        s = twin[0].stats
        out["host_twin_one_thread"] = {"whole_call_s": round(host_s, 3), "columns_and_backtrace_s": round((s["total_ms"] - s["host_ms"]) / 1e3, 3),
                                       "identical_to_device": bool(all(a.tobytes() == b.tobytes() for a, b in zip(twin, got)))}
    line = json.dumps(out)
    print(line, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", type=int, default=2000)
    ap.add_argument("--positions", type=int, default=100_000)
    ap.add_argument("--ploidies", type=int, nargs="*", default=[6, 4])
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "haplothread", "bench.jsonl"))
    a = ap.parse_args()
    for ploidy in a.ploidies:
        if a.sections:
            measure("sections_of_500", ploidy, problems_of(ploidy, a.sections, 500), a.repeat, not a.no_host, a.out)
        if a.positions:
            measure("one_section", ploidy, problems_of(ploidy, 1, a.positions), a.repeat, not a.no_host, a.out)


if __name__ == "__main__":
    main()
