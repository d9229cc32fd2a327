#!/usr/bin/env python3
"""Haplotagphase at scale: the seeded long-read chromosome of tests/haplotagphase_cases.py (bench_problem: --reads reads, default 2 M, of
30 consecutive variants on average with a tail of reads of up to 20 000, over --variants variants, default 1 M) through
whatshap_amd.haplotagphase.tagphase_batch.  One warm-up call, then --repeat timed calls; prints one JSON line and appends it to
profiles/haplotagphase/bench.jsonl (--out): reads, entries and variants of the problem, the whole call (wall, from the numpy arrays to the
result arrays), the library's split (host: validation, phase sets; upload / kernel / download from HIP events), median and min - max over
the repeats, entries/s of the kernels and of the whole call.
Next to the kernel time, the byte floor: the entries are read twice (count and place: variant, id and, when placing, quality), the runs
are written once and read once (12 bytes per voting entry each way), the per-variant words and results -- set against the achieved rate
and against a device-to-device copy of as many bytes (a hipMemcpyAsync between HIP events; the copy itself reads and writes that many
bytes, so kernels at the speed of light of the memory system would take about half the copy's time).  And the debug library's host twin
on one thread (--no-host skips it).  Not a bench.py entry.

    python scripts/gpu_haplotagphase_bench.py [--reads 2000000] [--variants 1000000] [--repeat 5] [--no-host] [--table] [--out profiles/haplotagphase/bench.jsonl]
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

import haplotagphase_cases as hc  # noqa: E402
from gpu_haplotag_bench import copy_ms, spread  # noqa: E402
from whatshap_amd import haplotagphase as tp  # noqa: E402


def run(n_reads, n_variants, repeat, host, table, out_path):
    problem = hc.bench_problem(n_reads=n_reads, n_variants=n_variants)
    tp.tagphase_batch([problem], want_table=table)   # warm-up: code objects, the pools' blocks
    walls, stats = [], []
    got = None
    for _ in range(repeat):
        st = []
        t0 = time.perf_counter()
        got = tp.tagphase_batch([problem], want_table=table, stats=st)[0]
        walls.append((time.perf_counter() - t0) * 1e3)
        stats.append(st[0])
    s0 = stats[0]
    n_entries, n_voting, n_var, n_rd = s0["n_entries"], s0["n_voting"], s0["n_variants"], s0["n_reads"]
    # count reads variant + id (5 bytes an entry), place variant + id + quality (9); the runs go out and come back at 12 bytes a voting entry;
    # per variant: flags word, counter (written, scanned, read), prefix (written, read twice), cursor, the 32-byte result; per read 12 bytes, twice
    n_bytes = n_entries * (5 + 9) + n_voting * (12 + 12) + n_var * (4 + 3 * 4 + 3 * 4 + 4 + 32) + n_rd * 12 * 2
    kernel = spread([s["kernel_ms"] for s in stats])
    copies = spread(copy_ms(n_bytes, repeat))
    out = {
        "workload": "long_read_chromosome", "reads": int(n_rd), "entries": int(n_entries), "variants": int(n_var), "want_table": bool(table), "repeat": repeat,
        **{k: int(s0[k]) for k in ("n_voting", "n_skipped", "n_voted", "n_kept", "n_zero_total", "variants_class_a", "variants_class_b", "variants_class_c",
                                   "variants_many_phase_sets", "table_rows", "launches")},
        "whole_call_ms": spread(walls),
        "library": {k: spread([s[k] for s in stats]) for k in ("host_ms", "upload_ms", "kernel_ms", "download_ms", "total_ms")},
        "entries_per_s_kernel": n_entries / (kernel["median"] / 1e3),
        "entries_per_s_whole_call": n_entries / (statistics.median(walls) / 1e3),
        "byte_floor_of_the_kernels": int(n_bytes),
        "device_to_device_copy_of_that_many_bytes_ms": copies,
        "kernel_over_copy": round(kernel["median"] / copies["median"], 3),
        "kernel_gbytes_per_s": round(n_bytes / (kernel["median"] / 1e3) / 1e9, 1),
    }
    if host:
        t0 = time.perf_counter()
        twin = tp.tagphase_batch([problem], host=True, want_table=table)[0]
        host_s = time.perf_counter() - t0
        fields = tp.TagphaseResult.FIELDS + (tp.TagphaseResult.TABLE_FIELDS if table else ())
        out["host_twin_one_thread"] = {"whole_call_s": round(host_s, 3), "voting_s": round((twin.stats["total_ms"] - twin.stats["host_ms"]) / 1e3, 3),
                                       "identical_to_device": bool(all(np.array_equal(getattr(twin, f), getattr(got, f)) for f in fields))}
    line = json.dumps(out)
    print(line, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--variants", type=int, default=1_000_000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--table", action="store_true", help="with the vote table (11 launches instead of 7)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "haplotagphase", "bench.jsonl"))
    a = ap.parse_args()
    run(a.reads, a.variants, a.repeat, not a.no_host, a.table, a.out)


if __name__ == "__main__":
    main()
