#!/usr/bin/env python3
"""Haplotagging at scale: the seeded problems of tests/haplotag_cases.py through whatshap_amd.haplotag.haplotag_batch -- "long2": --reads
long reads (default 2 M) of 30 variants on average with a tail of reads of up to 20 000 (about 6.4e7 entries) at ploidy 2, "long4": the
same at ploidy 4, "linked": as many short linked reads (0 .. 3 variants, 20 reads per BX tag on average).  One warm-up call per problem,
then --repeat timed calls; prints one JSON line per problem and appends it to profiles/haplotag/bench.jsonl (--out): the whole call (wall,
from the numpy arrays to the result arrays), the library's split (host: validation, position lookup, grouping; upload / kernel / download
from HIP events), median and min - max over the repeats, entries/s of the kernel and of the whole call.
Measured against: a device-to-device copy of as many bytes as the kernels must read and write (entries, group records, the variants once,
results), a hipMemcpyAsync between HIP events on the same device, same repeats -- the copy itself reads and writes that many bytes,
so a kernel at the speed of light of the memory system would take about half the copy's time --; and the debug library's host twin on one
thread (--no-host skips it).  Not a bench.py entry.

    python scripts/gpu_haplotag_bench.py [--reads 2000000] [--repeat 5] [--no-host] [--only long2] [--out profiles/haplotag/bench.jsonl]
    python scripts/gpu_haplotag_bench.py --sweep [--reads 2000000] [--repeat 5] [--sweep-out profiles/haplotag/threshold_sweep.jsonl]
        (the class boundaries 64 / 4096 against alternatives, through the debug library's switches)
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

import haplotag_cases as hc  # noqa: E402
from whatshap_amd import haplotag  # noqa: E402


def spread(values):
    return {"median": round(statistics.median(values), 3), "min": round(min(values), 3), "max": round(max(values), 3)}


def copy_ms(n_bytes, repeat):
    """hipMemcpyAsync device-to-device of n_bytes between HIP events, through the HIP runtime the library itself uses."""
    import ctypes as C

    hip = C.CDLL("libamdhip64.so")

    def ok(status):
        if status != 0:
            raise RuntimeError(f"HIP call failed with status {status}")

    src, dst, a, b = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    ok(hip.hipMalloc(C.byref(src), C.c_size_t(n_bytes)))
    ok(hip.hipMalloc(C.byref(dst), C.c_size_t(n_bytes)))
    ok(hip.hipEventCreate(C.byref(a)))
    ok(hip.hipEventCreate(C.byref(b)))
    times = []
    try:
        ok(hip.hipMemset(src, 1, C.c_size_t(n_bytes)))
        for k in range(repeat + 1):   # the first copy is the warm-up
            ok(hip.hipEventRecord(a, None))
            ok(hip.hipMemcpyAsync(dst, src, C.c_size_t(n_bytes), 3, None))   # hipMemcpyDeviceToDevice
            ok(hip.hipEventRecord(b, None))
            ok(hip.hipEventSynchronize(b))
            ms = C.c_float()
            ok(hip.hipEventElapsedTime(C.byref(ms), a, b))
            if k:
                times.append(ms.value)
    finally:
        hip.hipEventDestroy(a)
        hip.hipEventDestroy(b)
        hip.hipFree(src)
        hip.hipFree(dst)
    return times


def run(kind, n_reads, repeat, host, out_path):
    problem = hc.bench_problem(kind, n_reads=n_reads)
    haplotag.haplotag_batch([problem])   # warm-up: code objects, the pools' blocks
    walls, stats = [], []
    got = None
    for _ in range(repeat):
        st = []
        t0 = time.perf_counter()
        got = haplotag.haplotag_batch([problem], stats=st)[0]
        walls.append((time.perf_counter() - t0) * 1e3)
        stats.append(st[0])
    s0 = stats[0]
    scored = s0["groups_class_a"] + s0["groups_class_b"] + s0["groups_class_c"]
    n_bytes = s0["n_entries"] * 8 + scored * (16 + 16) + problem.variant_position.size * 8
    kernel = spread([s["kernel_ms"] for s in stats])
    copies = spread(copy_ms(n_bytes, repeat))
    out = {
        "workload": kind, "reads": int(s0["n_reads"]), "ploidy": problem.ploidy, "repeat": repeat,
        **{k: int(s0[k]) for k in ("n_groups", "n_assigned", "n_multiple_phase_sets", "n_entries", "groups_class_a", "groups_class_b", "groups_class_c",
                                   "groups_many_phase_sets", "launches")},
        "whole_call_ms": spread(walls),
        "library": {k: spread([s[k] for s in stats]) for k in ("host_ms", "upload_ms", "kernel_ms", "download_ms", "total_ms")},
        "entries_per_s_kernel": s0["n_entries"] / (kernel["median"] / 1e3),
        "entries_per_s_whole_call": s0["n_entries"] / (statistics.median(walls) / 1e3),
        "bytes_read_and_written_by_the_kernels": int(n_bytes),
        "device_to_device_copy_of_that_many_bytes_ms": copies,
        "kernel_over_copy": round(kernel["median"] / copies["median"], 3),
        "kernel_gbytes_per_s": round(n_bytes / (kernel["median"] / 1e3) / 1e9, 1),
    }
    if host:
        t0 = time.perf_counter()
        twin = haplotag.haplotag_batch([problem], host=True)[0]
        host_s = time.perf_counter() - t0
        out["host_twin_one_thread"] = {"whole_call_s": round(host_s, 3), "scoring_s": round((twin.stats["total_ms"] - twin.stats["host_ms"]) / 1e3, 3),
                                       "identical_to_device": bool(np.array_equal(twin.haplotype, got.haplotype) and np.array_equal(twin.quality, got.quality)
                                                                   and np.array_equal(twin.phaseset, got.phaseset) and np.array_equal(twin.bx_start, got.bx_start))}
    line = json.dumps(out)
    print(line, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(line + "\n")


SWEEP = [(64, 4096), (8, 4096), (16, 4096), (32, 4096), (128, 4096), (256, 4096), (1024, 4096), (64, 256), (64, 1024), (64, 16384), (64, 1 << 30)]


def sweep(n_reads, repeat, out_path):
    """The class boundaries against alternatives, on the long-read problem at ploidy 2: the debug library reads WHAMD_HT_CLASS_A_MAX /
    WHAMD_HT_CLASS_B_MAX at every call (every kernel is correct for any group size; only the speed changes).  One line per setting:
    groups per class and the kernels' time from the library's HIP events, median and min - max; the first setting is the shipped one."""
    from whatshap_amd import _native

    _native.use_debug_library()
    problem = hc.bench_problem("long2", n_reads=n_reads)
    want = None
    for a_max, b_max in SWEEP:
        os.environ["WHAMD_HT_CLASS_A_MAX"], os.environ["WHAMD_HT_CLASS_B_MAX"] = str(a_max), str(b_max)
        haplotag.haplotag_batch([problem])
        stats, got = [], None
        for _ in range(repeat):
            st = []
            got = haplotag.haplotag_batch([problem], stats=st)[0]
            stats.append(st[0])
        if want is None:
            want = got
        same = bool(np.array_equal(got.haplotype, want.haplotype) and np.array_equal(got.quality, want.quality) and np.array_equal(got.phaseset, want.phaseset))
        s0 = stats[0]
        line = json.dumps({"workload": "long2", "reads": n_reads, "class_a_max": a_max, "class_b_max": b_max, "shipped": (a_max, b_max) == SWEEP[0],
                           "groups_class_a": int(s0["groups_class_a"]), "groups_class_b": int(s0["groups_class_b"]), "groups_class_c": int(s0["groups_class_c"]),
                           "launches": int(s0["launches"]), "kernel_ms": spread([s["kernel_ms"] for s in stats]), "results_equal_to_shipped_setting": same})
        print(line, flush=True)
        if out_path:
            os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
            with open(out_path, "a") as f:
                f.write(line + "\n")
    del os.environ["WHAMD_HT_CLASS_A_MAX"], os.environ["WHAMD_HT_CLASS_B_MAX"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--only", choices=("long2", "long4", "linked"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "haplotag", "bench.jsonl"))
    ap.add_argument("--sweep", action="store_true", help="instead: the class boundaries against alternatives (debug library)")
    ap.add_argument("--sweep-out", default=os.path.join(ROOT, "profiles", "haplotag", "threshold_sweep.jsonl"))
    a = ap.parse_args()
    if a.sweep:
        return sweep(a.reads, a.repeat, a.sweep_out)
    for kind in ("long2", "long4", "linked"):
        if a.only in (None, kind):
            run(kind, a.reads, a.repeat, not a.no_host, a.out)


if __name__ == "__main__":
    main()
