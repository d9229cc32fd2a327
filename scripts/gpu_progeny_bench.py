#!/usr/bin/env python3
"""Progeny marker scoring at scale: the seeded chromosome-sized problem of tests/progeny_cases.py (60 000 nodes x 200 progeny samples,
ploidy 4, scoring window 250: about 13.5 M stored entries, 2.7 G sample terms) and the same at half the nodes, through
whatshap_amd.progeny.  One warm-up call per size, then --repeat timed calls; prints one JSON line per size and appends it to
profiles/progeny/bench.jsonl (--out): the whole call (wall, from the numpy table to the result arrays), the library's split (host entry
lists, upload / kernel / download from HIP events; the rest of the library's wall time is the repack of the table and the copies of the
result), median and min - max over the repeats, sample terms/s and entries/s of the kernel and of the whole call.
Measured against: the debug library's host twin -- the reference's arithmetic, one thread -- on the entries of a fixed 1 % of the
anchors, scaled to all entries (--no-host skips it).  Not a bench.py entry.

    python scripts/gpu_progeny_bench.py [--nodes 60000] [--samples 200] [--repeat 5] [--no-host] [--out profiles/progeny/bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import progeny_cases as pc  # noqa: E402
from whatshap_amd import progeny  # noqa: E402


def spread(values):
    return {"median": round(statistics.median(values), 3), "min": round(min(values), 3), "max": round(max(values), 3)}


def run(n_nodes, n_samples, repeat, host, out_path):
    table, node_variant, alt, co, window = pc.large_problem(n_nodes=n_nodes, n_samples=n_samples)
    problem = progeny.ProgenyProblem(progeny.ProgenyGenotypeLikelihoods.from_array(table), node_variant, alt, co, window)
    progeny.score_variants_batch([problem])   # warm-up: code objects, the pools' blocks
    walls, stats = [], []
    got = None
    for _ in range(repeat):
        st = []
        t0 = time.perf_counter()
        got = progeny.score_variants_batch([problem], stats=st)[0]
        walls.append((time.perf_counter() - t0) * 1e3)
        stats.append(st[0])
    s0 = stats[0]
    kernel = spread([s["kernel_ms"] for s in stats])
    out = {
        "workload": f"{n_nodes}_nodes_x_{n_samples}_samples", "nodes": n_nodes, "samples": n_samples, "ploidy": 4, "window": window, "repeat": repeat,
        "entries": s0["n_entries"], "entries_inf": s0["n_inf"], "entries_reused": s0["n_reused"], "sample_terms": s0["n_sample_terms"],
        "launches": s0["launches"], "whole_call_ms": spread(walls),
        "library": {k: spread([s[k] for s in stats]) for k in ("host_ms", "upload_ms", "kernel_ms", "download_ms", "total_ms")},
        "sample_terms_per_s_kernel": s0["n_sample_terms"] / (kernel["median"] / 1e3),
        "entries_per_s_kernel": s0["n_entries"] / (kernel["median"] / 1e3),
        "sample_terms_per_s_whole_call": s0["n_sample_terms"] / (statistics.median(walls) / 1e3),
        "entries_per_s_whole_call": s0["n_entries"] / (statistics.median(walls) / 1e3),
    }
    if host:
        # the entries of every 100th anchor, on one host thread
        i, j, _ = got.arrays()
        pick = np.nonzero(j % 100 == 0)[0]
        t0 = time.perf_counter()
        stored, ref = progeny.score_entries_host(problem, j[pick], i[pick])
        host_s = time.perf_counter() - t0
        dev = got.scores_f64()[pick]
        fin = np.isfinite(ref)
        out["host_twin_one_thread"] = {
            "entries_scored": int(pick.size), "seconds": round(host_s, 3), "scaled_to_all_entries_s": round(host_s * i.size / pick.size, 2),
            "max_abs_difference_to_device": float(np.abs(dev[fin] - ref[fin]).max()), "bit_identical": int((dev.view(np.uint64) == ref.view(np.uint64)).sum()),
            "all_stored": bool(stored.all()),
        }
    line = json.dumps(out)
    print(line, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=60_000)
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "progeny", "bench.jsonl"))
    a = ap.parse_args()
    run(a.nodes // 2, a.samples, a.repeat, not a.no_host, a.out)
    run(a.nodes, a.samples, a.repeat, not a.no_host, a.out)


if __name__ == "__main__":
    main()
