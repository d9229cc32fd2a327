#!/usr/bin/env python3
"""The prior genotype likelihoods at scale: one seeded chromosome of --positions positions (default 1 M) and --reads reads (default 2 M)
of about 20 entries each (consecutive positions, a tenth of the inner ones dropped; 2 % of the alleles are neither 0 nor 1; qualities
0 .. 45) through whatshap_amd.genotype.prior_genotypes_batch with the regularised outputs.  One warm-up call, then --repeat timed calls;
prints one JSON line and appends it to profiles/prior_genotypes/bench.jsonl (--out): the problem's counts, the whole call (wall, from the
numpy arrays to the result arrays), the library's split (map: validation fused with the mapping of entry positions to columns, on the
host; upload / kernel / download from HIP events), median and min - max over the repeats, entries/s of the kernels and of the whole
call.  And the debug library's host twin on one thread (--no-host skips it), compared byte for byte.  Not a bench.py entry.

    python scripts/gpu_prior_genotypes_bench.py [--positions 1000000] [--reads 2000000] [--repeat 5] [--no-host] [--out profiles/prior_genotypes/bench.jsonl]
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


def bench_arrays(n_positions=1_000_000, n_reads=2_000_000, mean_entries=20, seed=2024):
    """(read_ptr, position, allele, quality) of the benchmark's reads over the positions 0 .. n_positions - 1, sorted by first position."""
    rng = np.random.default_rng(seed)
    length = np.clip(rng.poisson(mean_entries + 2, n_reads), 1, max(1, min(n_positions, 4 * mean_entries))).astype(np.int64)
    start = rng.integers(0, np.maximum(n_positions - length, 0) + 1)
    order = np.argsort(start, kind="stable")
    start, length = start[order], length[order]
    ptr = np.zeros(n_reads + 1, dtype=np.int64)
    np.cumsum(length, out=ptr[1:])
    within = np.arange(ptr[-1], dtype=np.int64) - np.repeat(ptr[:-1], length)
    position = np.repeat(start, length) + within
    keep = (rng.random(position.size) >= 0.1) | (within == 0) | (within == np.repeat(length, length) - 1)   # (first and last stay: they must be listed)
    read_of = np.repeat(np.arange(n_reads), length)[keep]
    position = position[keep]
    read_ptr = np.zeros(n_reads + 1, dtype=np.uint64)
    np.cumsum(np.bincount(read_of, minlength=n_reads), out=read_ptr[1:])
    allele = rng.integers(0, 2, position.size).astype(np.uint8)
    allele[rng.random(position.size) < 0.02] = 3
    quality = rng.integers(0, 46, position.size).astype(np.uint32)
    return read_ptr, position.astype(np.uint32), allele, quality


def spread(values):
    return {"median": round(statistics.median(values), 3), "min": round(min(values), 3), "max": round(max(values), 3)}


def run(n_positions, n_reads, repeat, host, out_path):
    from whatshap_amd import genotype as gt

    read_ptr, position, allele, quality = bench_arrays(n_positions, n_reads)
    gt_prob = 1.0 - (10 ** (-10 / 10.0))

    def call(**kw):
        problem = gt.PriorProblem(read_ptr, position, allele, quality, np.arange(n_positions, dtype=np.uint32), constant=1e-3, gt_prob=gt_prob, want_regularized=True)
        return gt.prior_genotypes_batch([problem], **kw)[0]

    call()   # warm-up: code objects, the pools' blocks
    walls, stats = [], []
    got = None
    for _ in range(repeat):
        st = []
        t0 = time.perf_counter()
        got = call(stats=st)
        walls.append((time.perf_counter() - t0) * 1e3)
        stats.append(st[0])
    s0 = stats[0]
    kernel = spread([s["kernel_ms"] for s in stats])
    out = {
        "workload": "one_chromosome", "repeat": repeat,
        **{k: int(s0[k]) for k in ("n_reads", "n_positions", "n_entries", "n_counted", "n_covered", "n_genotyped", "columns_class_a", "columns_class_b",
                                   "columns_class_c", "longest_run", "launches")},
        "whole_call_ms": spread(walls),
        "library": {k: spread([s[k] for s in stats]) for k in ("map_ms", "host_ms", "upload_ms", "kernel_ms", "download_ms", "total_ms")},
        "entries_per_s_kernel": s0["n_entries"] / (kernel["median"] / 1e3),
        "entries_per_s_whole_call": s0["n_entries"] / (statistics.median(walls) / 1e3),
    }
    if host:
        st = []
        t0 = time.perf_counter()
        twin = call(host=True, stats=st)
        host_s = time.perf_counter() - t0
        out["host_twin_one_thread"] = {"whole_call_s": round(host_s, 3), "chains_s": round((st[0]["total_ms"] - st[0]["host_ms"]) / 1e3, 3),
                                       "identical_to_device": bool(all(getattr(twin, f).tobytes() == getattr(got, f).tobytes() for f in ("gl", "genotype", "reg", "reg_genotype")))}
    line = json.dumps(out)
    print(line, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=1_000_000)
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prior_genotypes", "bench.jsonl"))
    a = ap.parse_args()
    run(a.positions, a.reads, a.repeat, not a.no_host, a.out)


if __name__ == "__main__":
    main()
