#!/usr/bin/env python3
"""Allele detection by re-alignment at scale: a seeded workload of 200 000 variants over a 20 Mb synthetic reference (90 % SNV, 8 % indels
of 1 - 20 bp, 2 % multi-allelic), reads of 10 - 20 kb with 1 % errors at coverage 20 (about 4 M (read, variant) jobs), through
whatshap_amd.realign.detect_alleles_batch from Python objects, in both cost models.  Prints one JSON line per model: jobs/s end to end,
the library's split (host walk, upload, kernel, download, result lists), the flattening of the Python objects, and whether the result
equals the debug library's host restatement.  Not a bench.py entry.

    python scripts/gpu_realign_bench.py [--variants 200000] [--genome 20000000] [--coverage 20] [--no-check]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from whatshap_amd import realign  # noqa: E402
from whatshap_amd.synthetic import realign_workload  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", type=int, default=200_000)
    ap.add_argument("--genome", type=int, default=20_000_000)
    ap.add_argument("--coverage", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--no-check", action="store_true")
    a = ap.parse_args()
    t0 = time.perf_counter()
    ref, variants, reads = realign_workload(a.variants, a.genome, a.coverage, seed=11)
    print(json.dumps({"workload_s": round(time.perf_counter() - t0, 2), "reads": len(reads), "variants": len(variants)}), flush=True)
    for use_affine in (False, True):
        kw = dict(use_affine=True, gap_start=10, gap_extend=7, default_mismatch=15.1) if use_affine else {}
        realign.detect_alleles_batch(variants[:2000], reads[:50], ref, **kw)   # warm-up: library, device, pools
        best = None
        for _ in range(a.repeat):
            t = time.perf_counter()
            got, stats = realign.detect_alleles_batch(variants, reads, ref, with_stats=True, **kw)
            wall = time.perf_counter() - t
            if best is None or wall < best[0]:
                best = (wall, stats)
        wall, stats = best
        line = {"model": "affine" if use_affine else "unit", "jobs": stats["n_jobs"], "pairs": stats["n_pairs"], "results": stats["n_results"],
                "end_to_end_s": round(wall, 4), "jobs_per_s": round(stats["n_jobs"] / wall), "library_ms": round(stats["total_ms"], 2),
                "python_flatten_and_lists_ms": round(wall * 1e3 - stats["total_ms"], 2),
                **{k: round(stats[k], 3) for k in ("host_walk_ms", "upload_ms", "kernel_ms", "download_ms", "host_finish_ms")}}
        if not a.no_check:
            t = time.perf_counter()
            want = realign.detect_alleles_batch(variants, reads, ref, host=True, **kw)
            line["host_path_s"] = round(time.perf_counter() - t, 2)
            line["equals_host_path"] = got == want
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
