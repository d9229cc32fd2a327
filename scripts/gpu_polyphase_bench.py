#!/usr/bin/env python3
"""Polyphase read scoring at scale: a seeded long-read-like tetraploid block (50 000 reads of 20 - 300 variants over 40 000 positions, a
read every 2 500 spanning 20 000 variants: about 10 M candidate pairs) and a batch of 2 000 small blocks, through
whatshap_amd.polyphase.  Prints one JSON line per workload: pairs/s and pair-positions/s (shared positions summed over the candidate
pairs) inside the library (pair loop on the device, HIP events) and end to end from CSR arrays (AlleleMatrix + scoreReadset + result
arrays, wall), the library's split, and whether the result equals the debug library's host pair loop.  Not a bench.py entry.

    python scripts/gpu_polyphase_bench.py [--reads 50000] [--positions 40000] [--repeat 3] [--no-check]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from polyphase_cases import random_block  # noqa: E402
from whatshap_amd import polyphase  # noqa: E402


def run(name, blocks, min_overlap, ploidy, err, repeat, check):
    best = None
    for _ in range(repeat):
        t0 = time.perf_counter()
        ms = [polyphase.AlleleMatrix.from_csr(*b) for b in blocks]
        stats = []
        got = polyphase.score_readsets_batch(ms, min_overlap, ploidy, err, stats=stats)
        arrays = [g.arrays() for g in got]
        wall = time.perf_counter() - t0
        if best is None or wall < best[0]:
            best = (wall, stats, arrays, ms)
    wall, stats, arrays, ms = best
    s0 = stats[0]
    cand = sum(s["n_candidates"] for s in stats)
    pair_pos = sum(s["n_pair_positions"] for s in stats)
    device_ms = s0["kernel_ms"]
    out = {
        "workload": name, "matrices": len(blocks), "reads": sum(s["n_reads"] for s in stats), "candidate_pairs": cand,
        "entries": sum(s["n_entries"] for s in stats), "err": s0["err"],
        "library": {k: round(s0[k], 3) for k in ("host_ms", "upload_ms", "kernel_ms", "download_ms", "total_ms")},
        "pairs_per_s_device": cand / (device_ms / 1e3) if device_ms else None,
        "pairs_per_s_library": cand / (s0["total_ms"] / 1e3),
        "pairs_per_s_end_to_end": cand / wall,
        "end_to_end_s": round(wall, 4),
    }
    out["pair_positions"] = pair_pos
    out["pair_positions_per_s_device"] = pair_pos / (device_ms / 1e3) if device_ms else None
    if check:
        host = polyphase.score_readsets_batch(ms, min_overlap, ploidy, err, host=True)
        out["equals_host"] = all(np.array_equal(x, y) for h, a in zip(host, arrays) for x, y in zip(h.arrays(), a))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50_000)
    ap.add_argument("--positions", type=int, default=40_000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--no-check", action="store_true")
    a = ap.parse_args()
    big = [random_block(1, a.reads, a.positions, ploidy=4, n_alleles=2, min_len=20, max_len=300, long_every=2_500, long_len=20_000)]
    run("long_read_block", big, 2, 4, 0.07, a.repeat, not a.no_check)
    small = [random_block(1000 + b, 100 + b % 200, 400, ploidy=4, n_alleles=2, min_len=5, max_len=60) for b in range(2000)]
    run("batch_2000_blocks", small, 2, 4, 0.07, a.repeat, not a.no_check)


if __name__ == "__main__":
    main()
