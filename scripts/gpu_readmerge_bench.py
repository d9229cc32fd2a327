#!/usr/bin/env python3
"""The read merging at scale: one chromosome of long reads before the selection (tests/readmerge_cases.py, bench_reads) through
whatshap_amd.readmerge.merge_batch.  The read set is the phase benchmark's headline, whatshap_amd.synthetic.synthetic_block(200 000
variants, coverage 20): about 100 000 reads, one every 2 variants, each of 40 consecutive variants of which 10 % of the interior ones are
dropped (36 entries on average), 2 % allele errors, phred 5 .. 40 -- with positions equal to the variant indices, so that a read's window
(begin + len, a position plus a count) is its own span and every read is compared with the 15 to 20 reads that begin inside it; at the
benchmark's spacing of 1000 the reference compares no pair.  Thresholds of the command line's defaults: error rate 0.15, maximum error
rate 0.25, 10^6 and 10^3 (thr_diff 5, thr_neg_diff 3).

One warm-up call, then --repeat timed calls; prints one JSON line and appends it to profiles/readmerge/bench.jsonl (--out): the counts,
the whole call (wall, from the numpy arrays to the result arrays), the library's split (host preparation; upload / kernel / download from
HIP events; the pairs' kernel time on its own; the components on the host), median and min - max over the repeats, pairs/s of the pair
kernels.  Next to the pair kernels' time, their byte floor -- per pair the partner's 16-byte record, one 8-byte word of each read (a
36-entry read is one word; j's record and word are shared by the neighbouring lanes), 8 bytes written (flag, mismatches), the scan's 4
read and 4 written, the flag read again; per blue pair 20 bytes of edge -- set against a device-to-device copy of as many bytes.  And the
debug library's host twin on one thread (--no-host skips it).  Not a bench.py entry.

    python scripts/gpu_readmerge_bench.py [--variants 200000] [--coverage 20] [--repeat 5] [--no-host] [--out profiles/readmerge/bench.jsonl]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import readmerge_cases as rc  # noqa: E402
from gpu_haplotag_bench import copy_ms, spread  # noqa: E402
from whatshap_amd import readmerge as rm  # noqa: E402

ERROR_RATE, MAX_ERROR_RATE, POSITIVE, NEGATIVE = 0.15, 0.25, 1000000, 1000


def run(n_variants, coverage, repeat, host, out_path):
    read_ptr, position, allele, quality = rc.bench_reads(n_variants=n_variants, coverage=coverage)
    thr_diff, thr_neg_diff = rm.thresholds(ERROR_RATE, POSITIVE, NEGATIVE)
    rm.merge_batch([rm.MergeProblem(read_ptr, position, allele, quality, thr_diff, thr_neg_diff, MAX_ERROR_RATE)])   # warm-up: code objects, the pools' blocks
    walls, stats = [], []
    got = None
    for _ in range(repeat):
        st = []
        t0 = time.perf_counter()
        problem = rm.MergeProblem(read_ptr, position, allele, quality, thr_diff, thr_neg_diff, MAX_ERROR_RATE)
        got = rm.merge_batch([problem], want_edges=True, stats=st)[0]
        walls.append((time.perf_counter() - t0) * 1e3)
        stats.append(st[0])
    s0 = stats[0]
    n_pairs, n_blue = s0["n_pairs"], s0["n_blue"]
    n_bytes = n_pairs * (16 + 8 + 8 + 8 + 4 + 4 + 4) + n_blue * 20 + s0["n_reads"] * (16 + 4 + 4)
    pair_kernel = spread([s["pair_kernel_ms"] for s in stats])
    copies = spread(copy_ms(n_bytes, repeat))
    out = {
        "workload": "synthetic_block_positions_as_indices", "variants": n_variants, "coverage": coverage, "repeat": repeat,
        "thr_diff": thr_diff, "thr_neg_diff": thr_neg_diff, "max_error_rate": MAX_ERROR_RATE,
        **{k: int(s0[k]) for k in ("n_reads", "n_entries", "n_pairs", "n_blue", "n_not_blue", "n_merged_components", "n_merged_entries", "n_super_entries", "launches")},
        "merged_reads_out": int(np.count_nonzero(got.component_size == 1) + s0["n_merged_components"]),
        "whole_call_ms": spread(walls),
        "library": {k: spread([s[k] for s in stats]) for k in ("host_ms", "upload_ms", "kernel_ms", "pair_kernel_ms", "download_ms", "components_ms", "total_ms")},
        "pairs_per_s_pair_kernels": n_pairs / (pair_kernel["median"] / 1e3),
        "reads_per_s_whole_call": s0["n_reads"] / (statistics.median(walls) / 1e3),
        "byte_floor_of_the_pair_kernels": int(n_bytes),
        "device_to_device_copy_of_that_many_bytes_ms": copies,
        "pair_kernels_over_copy": round(pair_kernel["median"] / copies["median"], 3),
    }
    if host:
        problem = rm.MergeProblem(read_ptr, position, allele, quality, thr_diff, thr_neg_diff, MAX_ERROR_RATE)
        t0 = time.perf_counter()
        twin = rm.merge_batch([problem], host=True, want_edges=True)[0]
        host_s = time.perf_counter() - t0
        fields = rm.MergeResult.FIELDS + rm.MergeResult.EDGE_FIELDS
        out["host_twin_one_thread"] = {"whole_call_s": round(host_s, 3),
                                       "pairs_and_sums_s": round((twin.stats["total_ms"] - twin.stats["host_ms"] - twin.stats["components_ms"]) / 1e3, 3),
                                       "identical_to_device": bool(all(np.array_equal(getattr(twin, f), getattr(got, f)) for f in fields))}
    line = json.dumps(out)
    print(line, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", type=int, default=200_000)
    ap.add_argument("--coverage", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "readmerge", "bench.jsonl"))
    a = ap.parse_args()
    run(a.variants, a.coverage, a.repeat, not a.no_host, a.out)


if __name__ == "__main__":
    main()
