#!/usr/bin/env python3
"""Progeny scoring from allele depths at scale: the chromosome-sized problem of scripts/gpu_progeny_bench.py (60 000 nodes x 200 progeny
samples, ploidy 4, scoring window 250; tests/progeny_cases.large_problem gives the nodes and their types) with seeded depths
(tests/progeny_gl_cases.large_depths, mean depth 30), two ways in one sitting:

  depths  whatshap_amd.progeny.score_variants_from_depths: depths up, the likelihood kernel writes the planes, the pair kernel scores them
  table   whatshap_amd.progeny.score_variants_batch on the float table of the same likelihoods (made once, outside the timing, by
          offspring_gl_batch): the table repacked on the host and uploaded -- the path scripts/gpu_progeny_bench.py times

One warm-up call per path, then --repeat timed calls each; prints one JSON line per path and appends it to
profiles/progeny/bench_gl.jsonl (--out): the whole call (wall, from the numpy arrays to the result arrays) and the library's split (host
entry lists, upload / kernel / download from HIP events), median and min - max over the repeats, and the bytes uploaded.  The two paths
must give the same entries and bits; the script fails otherwise.  --table-only times nothing but the table path (what a build without
the depth calls can run: it then makes the table with numpy's own arithmetic -- the values differ in the last bits, the work does not).
Not a bench.py entry.

    python scripts/gpu_progeny_gl_bench.py [--nodes 60000] [--samples 200] [--repeat 5] [--table-only] [--build NAME] [--out profiles/progeny/bench_gl.jsonl]
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
import progeny_gl_cases as gc  # noqa: E402
from whatshap_amd import progeny  # noqa: E402


def spread(values):
    return {"median": round(statistics.median(values), 3), "min": round(min(values), 3), "max": round(max(values), 3)}


def timed(call, repeat):
    call()   # warm-up: code objects, the pools' blocks
    walls, stats, got = [], [], None
    for _ in range(repeat):
        st = []
        t0 = time.perf_counter()
        got = call(st)
        walls.append((time.perf_counter() - t0) * 1e3)
        stats.append(st[0])
    return got, walls, stats


def numpy_table(ref, alt, node_variant, alt_count, co_alt_count, ploidy, error_rate):
    """The likelihood table in numpy's double arithmetic (logs): for --table-only, where no library call makes it."""
    priors = np.array(progeny.compute_gt_likelihood_priors(ploidy))
    g = np.arange(ploidy + 1) / ploidy
    p = (1 - g) * error_rate + g * (1 - error_rate)
    with np.errstate(divide="ignore"):
        logw = alt.T[:, :, None] * np.log(p) + ref.T[:, :, None] * np.log(1 - p) + np.log(priors[alt_count, co_alt_count])[:, None, :]
    w = np.exp(logw - logw.max(axis=2, keepdims=True))
    table = (w / w.sum(axis=2, keepdims=True)).astype(np.float32)
    table[(ref + alt).T < ploidy] = -1.0
    return np.ascontiguousarray(table[node_variant])


def report(build, path, n_nodes, n_samples, window, repeat, walls, stats, upload_bytes, out_path):
    s0 = stats[0]
    out = {"build": build, "path": path, "workload": f"{n_nodes}_nodes_x_{n_samples}_samples", "nodes": n_nodes, "samples": n_samples, "ploidy": 4, "window": window,
           "repeat": repeat, "entries": s0["n_entries"], "sample_terms": s0["n_sample_terms"], "launches": s0["launches"], "upload_bytes": upload_bytes,
           "whole_call_ms": spread(walls),
           "library": {k: spread([s[k] for s in stats]) for k in ("host_ms", "upload_ms", "kernel_ms", "download_ms", "total_ms")}}
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
    ap.add_argument("--table-only", action="store_true")
    ap.add_argument("--build", default="this commit", help="recorded in the line: which build of the library ran")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "progeny", "bench_gl.jsonl"))
    a = ap.parse_args()
    ploidy, error_rate = 4, 0.06
    _, node_variant, alt_count, co_alt_count, window = pc.large_problem(n_nodes=a.nodes, n_samples=2)   # (its table is not used)
    ref, alt = gc.large_depths(alt_count, co_alt_count, n_samples=a.samples, ploidy=ploidy, error_rate=error_rate)
    entry_bytes = None
    fused = None
    if not a.table_only:
        depths = progeny.DepthProblem(ref, alt, ploidy, error_rate, node_row=node_variant, priors=progeny.compute_gt_likelihood_priors(ploidy),
                                      row_alt_count=alt_count, row_co_alt_count=co_alt_count, node_variant=node_variant, alt_count=alt_count,
                                      co_alt_count=co_alt_count, scoring_window=window)
        fused, walls, stats = timed(lambda st=None: progeny.score_variants_from_depths([depths], stats=st)[0], a.repeat)
        entry_bytes = 9 * stats[0]["n_entries"]
        report(a.build, "depths", a.nodes, a.samples, window, a.repeat, walls, stats, entry_bytes + ref.nbytes + alt.nbytes + node_variant.nbytes + 4 * alt_count.size,
               a.out)
        table = progeny.offspring_gl_batch([depths])[0]
    else:
        table = progeny.ProgenyGenotypeLikelihoods.from_array(numpy_table(ref, alt, node_variant, alt_count, co_alt_count, ploidy, error_rate))
    problem = progeny.ProgenyProblem(table, node_variant, alt_count, co_alt_count, window)
    unfused, walls, stats = timed(lambda st=None: progeny.score_variants_batch([problem], stats=st)[0], a.repeat)
    report(a.build, "table", a.nodes, a.samples, window, a.repeat, walls, stats, 9 * stats[0]["n_entries"] + 12 * a.nodes * a.samples, a.out)
    if fused is not None:
        for u, v in zip(fused.arrays(), unfused.arrays()):
            assert np.array_equal(u.view(np.uint32), v.view(np.uint32)), "the two paths differ"
        assert np.array_equal(fused.scores_f64().view(np.uint64), unfused.scores_f64().view(np.uint64)), "the two paths differ"


if __name__ == "__main__":
    main()
