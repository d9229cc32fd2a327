#!/usr/bin/env python3
"""Writes tests/golden/haplothread_cases.json.gz: what the reference's HaploThreader makes of the cases of tests/haplothread_cases.py (run
only where the reference tree exists; the tests read the recorded data).

The reference's src/polyphase/haplothreader.cpp, tupleconverter.cpp and src/binomial.cpp are compiled with a small extern "C" wrapper
(written here, below) into a temporary directory outside the repository and loaded with ctypes.  The wrapper reaches the private
computeCoverage, getCoverageCost and getSwitchCostAllPerms by including the class's header with ``private`` defined away.  Nothing of the
reference is written out.

Recorded per case: the inputs (tests/haplothread_cases.py generates them); ``path``, what computePaths(blockStarts, covMap, alleleDepths)
returns; ``smoothed``, computeCoverage's clusterCoverage; ``path_cost``, getCoverageCost of every path tuple (float, as hex); ``optimum``,
per section the cost of that path under the recurrence (score + switch) + cov, in float, with getSwitchCostAllPerms for the switch (as
hex): the reference's optimum.  For the small cases ``all_costs``: getCoverageCost of every tuple of every position in enumeration order.
``pipeline``: for the recorded cases of tests/golden/polythread_cases.json.gz with a ploidy of 2 .. 6, the reference's path over their
recorded cov_map and allele depths with run_threading's costs.  No case is dropped.
Usage: python tests/golden/make_haplothread_golden.py [/path/to/reference]
       python tests/golden/make_haplothread_golden.py /path/to/reference --baseline N
           (writes nothing: times the reference's threader, one thread, on the workloads of scripts/gpu_haplothread_bench.py scaled to N
           positions in all -- the figures of profiles/haplothread/cpu_baseline.md)
"""
import ctypes as C
import gzip
import json
import math
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "haplothread_cases.json.gz")
sys.path.insert(0, os.path.dirname(HERE))
import haplothread_cases as hc  # noqa: E402

WRAPPER = r"""
#include <cstdint>
#include <cmath>
#include <iostream>
#include <sstream>
#include <string>
#include <algorithm>
#include <limits>
#include <stdexcept>
#include <unordered_map>
#include <unordered_set>
#include <vector>
#define private public
#include "polyphase/haplothreader.h"
#undef private
typedef std::vector<std::unordered_map<GlobalClusterId, std::unordered_map<uint32_t, uint32_t>>> Depths;
static void inputs(unsigned n_pos, const unsigned long long* cov_ptr, const unsigned* cov, const unsigned long long* pc_ptr, const unsigned* pc_cluster,
                   const unsigned* pc_total, std::vector<std::vector<GlobalClusterId>>& cov_map, Depths& depths) {
    cov_map.resize(n_pos);
    depths.resize(n_pos);
    for (unsigned x = 0; x < n_pos; x++) {
        cov_map[x].assign(cov + cov_ptr[x], cov + cov_ptr[x + 1]);
        for (unsigned long long k = pc_ptr[x]; k < pc_ptr[x + 1]; k++) {
            depths[x][pc_cluster[k]];
            if (pc_total[k]) depths[x][pc_cluster[k]][0] = pc_total[k];
        }
    }
}
extern "C" {
void* ht_new(unsigned ploidy, double switch_cost, double affine, unsigned gap, unsigned row_limit) { return new HaploThreader(ploidy, switch_cost, affine, gap, row_limit); }
void ht_delete(void* h) { delete (HaploThreader*)h; }
// -1: std::out_of_range (a listed cluster without a depth row)
long long ht_paths(void* h, unsigned ploidy, unsigned n_pos, const unsigned long long* cov_ptr, const unsigned* cov, const unsigned long long* pc_ptr,
                   const unsigned* pc_cluster, const unsigned* pc_total, const unsigned* block_starts, unsigned n_starts, unsigned* path_out) {
    std::vector<std::vector<GlobalClusterId>> cov_map;
    Depths depths;
    inputs(n_pos, cov_ptr, cov, pc_ptr, pc_cluster, pc_total, cov_map, depths);
    try {
        auto path = ((HaploThreader*)h)->computePaths(std::vector<Position>(block_starts, block_starts + n_starts), cov_map, depths);
        for (size_t x = 0; x < path.size(); x++)
            for (unsigned i = 0; i < ploidy; i++) path_out[x * ploidy + i] = path[x][i];
        return (long long)path.size();
    } catch (const std::out_of_range&) {
        return -1;
    }
}
void ht_coverage(void* h, unsigned n_pos, const unsigned long long* cov_ptr, const unsigned* cov, const unsigned long long* pc_ptr, const unsigned* pc_cluster,
                 const unsigned* pc_total, unsigned* smoothed_out, unsigned* coverage_out) {
    std::vector<std::vector<GlobalClusterId>> cov_map;
    Depths depths;
    inputs(n_pos, cov_ptr, cov, pc_ptr, pc_cluster, pc_total, cov_map, depths);
    std::vector<uint32_t> coverage(n_pos, 0);
    std::vector<std::vector<uint32_t>> cluster_coverage(n_pos);
    ((HaploThreader*)h)->computeCoverage(depths, cov_map, coverage, cluster_coverage);
    for (unsigned x = 0; x < n_pos; x++) {
        coverage_out[x] = coverage[x];
        for (size_t k = 0; k < cluster_coverage[x].size(); k++) smoothed_out[cov_ptr[x] + k] = cluster_coverage[x][k];
    }
}
float ht_coverage_cost(void* h, const unsigned* local_ids, unsigned ploidy, unsigned coverage, const unsigned* cluster_coverage, unsigned n) {
    return ((HaploThreader*)h)->getCoverageCost(ClusterTuple(std::vector<LocalClusterId>(local_ids, local_ids + ploidy)), coverage,
                                                std::vector<uint32_t>(cluster_coverage, cluster_coverage + n));
}
float ht_switch_cost(void* h, const unsigned* before_sorted, const unsigned* now_sorted, unsigned ploidy) {
    return ((HaploThreader*)h)->getSwitchCostAllPerms(std::vector<GlobalClusterId>(before_sorted, before_sorted + ploidy),
                                                      std::vector<GlobalClusterId>(now_sorted, now_sorted + ploidy));
}
}
"""

SOURCES = ["polyphase/haplothreader.cpp", "polyphase/tupleconverter.cpp", "binomial.cpp"]
U32, U64 = C.POINTER(C.c_uint), C.POINTER(C.c_ulonglong)


def build_wrapper(ref_root, tmp):
    src = os.path.join(tmp, "wrapper.cpp")
    open(src, "w").write(WRAPPER)
    so = os.path.join(tmp, "libht.so")
    srcdir = os.path.join(ref_root, "src")
    subprocess.run(["g++", "-O2", "-std=c++14", "-shared", "-fPIC", "-I" + srcdir, src] + [os.path.join(srcdir, s) for s in SOURCES] + ["-o", so], check=True)
    L = C.CDLL(so)
    L.ht_new.restype = C.c_void_p
    L.ht_new.argtypes = [C.c_uint, C.c_double, C.c_double, C.c_uint, C.c_uint]
    L.ht_delete.argtypes = [C.c_void_p]
    L.ht_paths.restype = C.c_longlong
    L.ht_paths.argtypes = [C.c_void_p, C.c_uint, C.c_uint, U64, U32, U64, U32, U32, U32, C.c_uint, U32]
    L.ht_coverage.argtypes = [C.c_void_p, C.c_uint, U64, U32, U64, U32, U32, U32, U32]
    L.ht_coverage_cost.restype = C.c_float
    L.ht_coverage_cost.argtypes = [C.c_void_p, U32, C.c_uint, C.c_uint, U32, C.c_uint]
    L.ht_switch_cost.restype = C.c_float
    L.ht_switch_cost.argtypes = [C.c_void_p, U32, U32, C.c_uint]
    return L


def hex32(x):
    return float(np.float32(x)).hex()


def u32s(values):
    return (C.c_uint * max(len(values), 1))(*[int(v) for v in values])


def run_reference(L, case, arrays=None):
    """(path [n_pos][ploidy] or None where the reference throws, smoothed, coverage) of a case."""
    cov_ptr, cov, pc_ptr, pc_cluster, pc_total = arrays if arrays is not None else hc.arrays_of(case)
    n_pos, P = len(cov_ptr) - 1, case["ploidy"]
    h = L.ht_new(P, case["switch_cost"], case["affine_switch_cost"], case["max_gap"], 0)
    cov, pc_cluster, pc_total = (np.ascontiguousarray(a, dtype=np.uint32) for a in (cov, pc_cluster, pc_total))
    cov_ptr, pc_ptr = (np.ascontiguousarray(a, dtype=np.uint64) for a in (cov_ptr, pc_ptr))
    a = (n_pos, cov_ptr.ctypes.data_as(U64), cov.ctypes.data_as(U32), pc_ptr.ctypes.data_as(U64), pc_cluster.ctypes.data_as(U32), pc_total.ctypes.data_as(U32))
    path = np.zeros((n_pos, P), dtype=np.uint32)
    starts = u32s(case["block_starts"])
    got = L.ht_paths(h, P, *a, starts, len(case["block_starts"]), path.ctypes.data_as(U32))
    if got < 0:
        L.ht_delete(h)
        return None, None, None, None
    assert got == n_pos, (case["name"], got, n_pos)
    smoothed, coverage = np.zeros(len(cov), dtype=np.uint32), np.zeros(n_pos, dtype=np.uint32)
    L.ht_coverage(h, *a, smoothed.ctypes.data_as(U32), coverage.ctypes.data_as(U32))
    return h, path, smoothed, coverage


def record_case(L, case):
    rec = dict(case)
    h, path, smoothed, coverage = run_reference(L, case)
    assert h is not None, case["name"]
    P, cov_map = case["ploidy"], case["cov_map"]
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in cov_map])]).tolist()
    rec["path"] = path.tolist()
    rec["smoothed"] = smoothed.tolist()

    def cost_of(x, local):
        cc = smoothed[ptr[x]:ptr[x + 1]].tolist()
        return np.float32(L.ht_coverage_cost(h, u32s(local), P, int(coverage[x]), u32s(cc), len(cc)))

    path_cost = [cost_of(x, [cov_map[x].index(g) for g in path[x].tolist()]) for x in range(len(cov_map))]
    rec["path_cost"] = [hex32(c) for c in path_cost]
    optimum = []
    for start, end in hc.sections_of(case):
        score = np.float32(np.float32(0.0) + path_cost[start])
        for x in range(start + 1, end):
            switch = np.float32(L.ht_switch_cost(h, u32s(sorted(path[x - 1].tolist())), u32s(sorted(path[x].tolist())), P))
            score = np.float32(np.float32(score + switch) + path_cost[x])
        optimum.append(hex32(score))
    rec["optimum"] = optimum
    if case["small"]:
        rec["all_costs"] = [[hex32(cost_of(x, t)) for t in hc.enumerate_tuples(P, len(cov_map[x]))] for x in range(len(cov_map))]
    L.ht_delete(h)
    return rec


def pipeline_cases():
    """The recorded threading inputs of tests/golden/polythread_cases.json.gz as threader cases, with run_threading's costs."""
    with gzip.open(os.path.join(HERE, "polythread_cases.json.gz"), "rb") as f:
        recorded = json.loads(f.read().decode())["cases"]
    out = []
    for k, r in enumerate(recorded):
        if not 2 <= r["ploidy"] <= 6 or "cov_map" not in r or max(len(x) for x in r["cov_map"]) > 8:
            continue
        affine = math.ceil(float.fromhex(r["ratio"]) / 1.0)
        depths = [[[cid, sum(n for _, n in alleles)] for cid, alleles in position] for position in r["ad_after"]]
        out.append(dict(hc.case(r["name"], r["ploidy"], r["cov_map"], depths, float(4 * affine), float(affine), r["max_gap"]), index=k))
    return out


def baseline(ref_root, n_total):
    import time

    with tempfile.TemporaryDirectory() as tmp:
        L = build_wrapper(ref_root, tmp)
        for ploidy in (6, 4):
            for name, n_sections in (("sections_of_500", max(1, n_total // 500)), ("one_section", 1)):
                n_pos = 500 if n_sections > 1 else n_total
                t = 0.0
                for s in range(n_sections):
                    arrays = hc.bench_problem(ploidy, n_pos, seed=s)
                    case = {"name": name, "ploidy": ploidy, "switch_cost": 12.0, "affine_switch_cost": 3.0, "max_gap": 10, "block_starts": [0]}
                    t0 = time.perf_counter()
                    h, path, _, _ = run_reference(L, case, arrays)
                    t += time.perf_counter() - t0
                    L.ht_delete(h)
                print(json.dumps({"workload": name, "ploidy": ploidy, "sections": n_sections, "positions": n_sections * n_pos, "reference_s": round(t, 3),
                                  "includes": "computePaths and one further computeCoverage"}))


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("WHATSHAP_REFERENCE", "")
    if not ref_root or not os.path.isdir(os.path.join(ref_root, "src", "polyphase")):
        sys.exit("usage: make_haplothread_golden.py /path/to/reference (a WhatsHap source tree)")
    if len(sys.argv) > 3 and sys.argv[2] == "--baseline":
        return baseline(ref_root, int(sys.argv[3]))
    with tempfile.TemporaryDirectory() as tmp:
        L = build_wrapper(ref_root, tmp)
        cases = [record_case(L, c) for c in hc.all_cases()]
        pipeline = [record_case(L, c) for c in pipeline_cases()]
        missing = hc.case("missing_row", 2, [[1, 2], [1, 2]], [[[1, 5], [2, 5]], [[1, 5]]])
        assert run_reference(L, missing)[0] is None, "the reference did not throw for a listed cluster without a depth row"
    with gzip.GzipFile(OUT, "wb", mtime=0) as f:
        f.write(json.dumps({"cases": cases, "pipeline": pipeline}, separators=(",", ":")).encode())
    print(f"{len(cases)} cases + {len(pipeline)} pipeline cases, {sum(len(c['cov_map']) for c in cases)} positions -> {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
