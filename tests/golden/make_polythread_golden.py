#!/usr/bin/env python3
"""Writes tests/golden/polythread_cases.json.gz: what the reference's threading inputs are for the cases of tests/polythread_cases.py (run
only where the reference tree exists; the tests read the recorded data).

The reference's src/polyphase/allelematrix.cpp and the src/*.cpp it needs are compiled with a small extern "C" wrapper (written here,
below) into a temporary directory outside the repository and loaded with ctypes: AlleleMatrix(ReadSet*), extractSubMatrix, getNumPositions and
getRead are the reference's own.  The reference's own Python functions run against it: at generation time whatshap/polyphase/threading.py is parsed
and only ``get_allele_depths``, ``select_clusters``, ``compute_haplotypes`` and ``compute_readlength_snp_distance_ratio`` are executed,
with a stand-in for the one name they import (``defaultdict``).  Nothing of the reference is written out.

Recorded per case: the inputs (tests/polythread_cases.py generates them); ``ad`` and ``cons_lists`` as get_allele_depths returns them --
dicts as lists of pairs, so that the insertion orders are part of the record --; ``cov_map``; ``ad_after``, the allele depths as
select_clusters leaves them; the read length ratio; ``paths`` drawn here from cov_map with a seeded generator (repeats, a cluster id
without a list, one id in all slots) and the ``haplotypes`` compute_haplotypes makes of them.  For the case of a position without a
counted entry: the exception select_clusters raises.  For the select cases: the dicts handed in, cov_map and the dicts afterwards.
No case is dropped.
Usage: python tests/golden/make_polythread_golden.py [/path/to/reference]
       python tests/golden/make_polythread_golden.py /path/to/reference --baseline 20000
           (writes nothing: times the reference's own get_allele_depths + select_clusters on the first 20000 positions of the benchmark's
           block, one thread -- the figure of profiles/polythread/cpu_baseline.md)
"""
import __future__

import ast
import collections
import ctypes as C
import gzip
import json
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "polythread_cases.json.gz")
sys.path.insert(0, os.path.dirname(HERE))
import polythread_cases as pc  # noqa: E402

WRAPPER = r"""
#include <cstdint>
#include <string>
#include <vector>
#include "read.h"
#include "readset.h"
#include "polyphase/allelematrix.h"
extern "C" {
void* am_new(unsigned n_reads, const unsigned long long* read_ptr, const int* pos, const int* allele) {
    ReadSet* rs = new ReadSet();
    for (unsigned r = 0; r < n_reads; r++) {
        Read* read = new Read("r" + std::to_string(r), 60, 0, 0);
        for (unsigned long long x = read_ptr[r]; x < read_ptr[r + 1]; x++) read->addVariant(pos[x], allele[x], 10);
        rs->add(read);
    }
    AlleleMatrix* am = new AlleleMatrix(rs);
    delete rs;
    return am;
}
void am_delete(void* p) { delete (AlleleMatrix*)p; }
unsigned long long am_size(void* p) { return ((AlleleMatrix*)p)->size(); }
unsigned long long am_num_positions(void* p) { return ((AlleleMatrix*)p)->getNumPositions(); }
void* am_extract(void* p, const unsigned* positions, unsigned n_positions, const unsigned* reads, unsigned n_reads, int remove_empty) {
    return ((AlleleMatrix*)p)->extractSubMatrix(std::vector<uint32_t>(positions, positions + n_positions), std::vector<uint32_t>(reads, reads + n_reads),
                                                remove_empty != 0);
}
unsigned am_read(void* p, unsigned r, unsigned* pos_out, int* allele_out, unsigned cap) {
    auto row = ((AlleleMatrix*)p)->getRead(r);
    for (unsigned x = 0; x < row.size() && x < cap; x++) {
        pos_out[x] = row[x].first;
        allele_out[x] = (int)row[x].second;
    }
    return (unsigned)row.size();
}
}
"""

SOURCES = ["read.cpp", "readset.cpp", "entry.cpp", "indexset.cpp", "polyphase/allelematrix.cpp"]


def build_wrapper(ref_root, tmp):
    src = os.path.join(tmp, "wrapper.cpp")
    open(src, "w").write(WRAPPER)
    so = os.path.join(tmp, "libam.so")
    srcdir = os.path.join(ref_root, "src")
    subprocess.run(["g++", "-O2", "-std=c++14", "-shared", "-fPIC", "-I" + srcdir, src] + [os.path.join(srcdir, s) for s in SOURCES] + ["-o", so], check=True)
    L = C.CDLL(so)
    L.am_new.restype = C.c_void_p
    L.am_new.argtypes = [C.c_uint, C.POINTER(C.c_ulonglong), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.am_delete.argtypes = [C.c_void_p]
    for name in ("am_size", "am_num_positions"):
        getattr(L, name).restype = C.c_ulonglong
        getattr(L, name).argtypes = [C.c_void_p]
    L.am_extract.restype = C.c_void_p
    L.am_extract.argtypes = [C.c_void_p, C.POINTER(C.c_uint), C.c_uint, C.POINTER(C.c_uint), C.c_uint, C.c_int]
    L.am_read.restype = C.c_uint
    L.am_read.argtypes = [C.c_void_p, C.c_uint, C.POINTER(C.c_uint), C.POINTER(C.c_int), C.c_uint]
    return L


class RefMatrix:
    """The compiled reference class behind the method names the reference's Python uses."""

    def __init__(self, L, handle):
        self.L, self.h = L, handle

    @classmethod
    def from_csr(cls, L, read_ptr, pos, alle):
        n = len(read_ptr) - 1
        return cls(L, L.am_new(n, (C.c_ulonglong * len(read_ptr))(*[int(x) for x in read_ptr]), (C.c_int * max(len(pos), 1))(*[int(x) for x in pos]),
                               (C.c_int * max(len(alle), 1))(*[int(x) for x in alle])))

    @classmethod
    def from_case(cls, L, case):
        """AlleleMatrix(ReadSet*) takes no read without variants: a case with one is made as the reference makes such matrices, by
        extractSubMatrix without removeEmpty, from a matrix in which the empty reads have one entry at a position behind the block."""
        if all(case["reads"]):
            return cls.from_csr(L, *pc.csr_of(case))
        n_pos, n_reads = case["n_pos"], len(case["reads"])
        padded = dict(case, reads=[row if row else [[n_pos, 0]] for row in case["reads"]])
        whole = cls.from_csr(L, *pc.csr_of(padded))
        part = cls(L, L.am_extract(whole.h, (C.c_uint * n_pos)(*range(n_pos)), n_pos, (C.c_uint * n_reads)(*range(n_reads)), n_reads, 0))
        whole.close()
        return part

    def close(self):
        self.L.am_delete(self.h)

    def __len__(self):
        return self.L.am_size(self.h)

    def getNumPositions(self):
        return self.L.am_num_positions(self.h)

    def getRead(self, r):
        cap = 4096
        pos, alle = (C.c_uint * cap)(), (C.c_int * cap)()
        n = self.L.am_read(self.h, r, pos, alle, cap)
        assert n <= cap
        return [(pos[x], alle[x]) for x in range(n)]

    def __iter__(self):
        return (self.getRead(r) for r in range(len(self)))


WANTED = ("get_allele_depths", "select_clusters", "compute_haplotypes", "compute_readlength_snp_distance_ratio")


def load_reference_functions(ref_root):
    """The four functions of the reference's threading.py, compiled from its own text at run time (annotations are not evaluated)."""
    path = os.path.join(ref_root, "whatshap", "polyphase", "threading.py")
    tree = ast.parse(open(path).read(), filename=path)
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in WANTED]
    assert sorted(n.name for n in keep) == sorted(WANTED)
    ns = {"defaultdict": collections.defaultdict}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec", flags=__future__.annotations.compiler_flag), ns)
    return ns


def pairs(dicts, leaf):
    """A list over positions of dicts over clusters, as lists of pairs in dict order."""
    return [[[int(cid), leaf(v)] for cid, v in d.items()] for d in dicts]


def depth_pairs(dicts):
    return pairs(dicts, lambda d: [[int(a), int(n)] for a, n in d.items()])


def draw_paths(rng, cov_map, ploidy, n_clusters, flavour):
    paths = []
    for x, clusters in enumerate(cov_map):
        if flavour == 0:      # from cov_map, with repeats
            paths.append([rng.choice(clusters) for _ in range(ploidy)])
        elif flavour == 1:    # one id in all slots
            paths.append([rng.choice(clusters)] * ploidy)
        else:                 # now and then a cluster from anywhere (it may have no list here), or an id no cluster has
            paths.append([rng.choice(clusters) if rng.random() < 0.6 else rng.randrange(n_clusters + 3) for _ in range(ploidy)])
    return paths


def record_case(L, ns, case, index):
    am = RefMatrix.from_case(L, case)
    assert am.getNumPositions() == case["n_pos"]
    rec = dict(case)
    ad, cons = ns["get_allele_depths"](am, case["clustering"], case["ploidy"])
    rec["ad"] = depth_pairs(ad)
    rec["cons_lists"] = pairs(cons, lambda picks: [int(a) for a in picks])
    rec["ratio"] = float(ns["compute_readlength_snp_distance_ratio"](am)).hex()
    try:
        cov_map = ns["select_clusters"](ad, case["ploidy"], case["max_gap"])
    except IndexError:
        rec["raises"] = "IndexError"
        am.close()
        return rec
    rec["cov_map"] = [[int(c) for c in clusters] for clusters in cov_map]
    rec["ad_after"] = depth_pairs(ad)
    rng = random.Random(9000 + index)
    rec["paths"], rec["haplotypes"] = [], []
    for flavour in range(3):
        paths = draw_paths(rng, cov_map, case["ploidy"], len(case["clustering"]), flavour)
        rec["paths"].append(paths)
        rec["haplotypes"].append([[int(a) for a in h] for h in ns["compute_haplotypes"](paths, cons, case["ploidy"])])
    am.close()
    return rec


def record_select_case(ns, case):
    ad = [{cid: {a: n for a, n in alleles} for cid, alleles in position} for position in case["depths"]]
    rec = dict(case)
    rec["cov_map"] = [[int(c) for c in clusters] for clusters in ns["select_clusters"](ad, case["ploidy"], case["max_gap"])]
    rec["ad_after"] = depth_pairs(ad)
    return rec


def baseline(ref_root, n_pos):
    """The reference's get_allele_depths + select_clusters on the compiled matrix: the first n_pos positions of pc.bench_arrays()."""
    import time

    ns = load_reference_functions(ref_root)
    full = pc.bench_arrays()
    read_ptr, pos, alle, clustering = pc.prefix_of(full, n_pos)
    with tempfile.TemporaryDirectory() as tmp:
        L = build_wrapper(ref_root, tmp)
        am = RefMatrix.from_csr(L, read_ptr.tolist(), pos.tolist(), alle.tolist())
        cl = [c.tolist() for c in clustering]
        t0 = time.perf_counter()
        ad, cons = ns["get_allele_depths"](am, cl, pc.BENCH["ploidy"])
        t1 = time.perf_counter()
        cov_map = ns["select_clusters"](ad, pc.BENCH["ploidy"], pc.BENCH["max_gap"])
        t2 = time.perf_counter()
    print(json.dumps({"positions_total": int((int(full[1].max()) - 100) // 7 + 1), "entries_total": int(full[0][-1]), "positions_timed": len(cov_map),
                      "reads_timed": len(read_ptr) - 1, "entries_timed": int(read_ptr[-1]), "get_allele_depths_s": round(t1 - t0, 3),
                      "select_clusters_s": round(t2 - t1, 3)}))


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("WHATSHAP_REFERENCE", "")
    if not ref_root or not os.path.isdir(os.path.join(ref_root, "src", "polyphase")):
        sys.exit("usage: make_polythread_golden.py /path/to/reference (a WhatsHap source tree)")
    if len(sys.argv) > 3 and sys.argv[2] == "--baseline":
        return baseline(ref_root, int(sys.argv[3]))
    ns = load_reference_functions(ref_root)
    with tempfile.TemporaryDirectory() as tmp:
        L = build_wrapper(ref_root, tmp)
        cases = [record_case(L, ns, case, k) for k, case in enumerate(pc.all_cases())]
        uncovered = record_case(L, ns, pc.uncovered_case(), len(cases))
    assert uncovered.get("raises") == "IndexError" and not any("raises" in c for c in cases)
    select = [record_select_case(ns, case) for case in pc.select_cases()]
    readded = sum(1 for c in cases for before, after in zip(c["ad"], c["ad_after"]) for row in after if row[0] not in [b[0] for b in before])
    emptied = sum(1 for c in cases for before, after in zip(c["ad"], c["ad_after"]) for (cid, d), (cid2, d2) in zip(before, after) if d and not d2)
    assert emptied > 0, "no re-added cluster with a non-empty depth row was recorded"
    with gzip.GzipFile(OUT, "wb", mtime=0) as f:
        f.write(json.dumps({"cases": cases, "uncovered": uncovered, "select": select, "emptied_rows": emptied}, separators=(",", ":")).encode())
    print(f"{len(cases)} cases + 1 refused + {len(select)} select cases, {sum(c['n_pos'] for c in cases)} positions, {readded} re-added without a row, "
          f"{emptied} emptied rows -> {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
