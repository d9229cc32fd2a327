#!/usr/bin/env python3
"""Writes tests/golden/reorder_cases.json.gz: what the reference's polyphase reordering returns for the cases of tests/reorder_cases.py
(run only where the reference tree exists; the tests read the recorded data).

The reference's src/polyphase/allelematrix.cpp and the src/*.cpp it needs are compiled with a small extern "C" wrapper (written here,
below) into a temporary directory outside the repository and loaded with ctypes: AlleleMatrix(ReadSet*), getFirstPos, getLastPos,
extractSubMatrix and getRead are the reference's own.  The reference's own Python functions run against it: at generation time
whatshap/polyphase/reorder.py is parsed and only ``run_reordering``, ``compute_link_likelihoods``, ``get_heterozygous_pos_for_haps``,
``find_breakpoints``, ``get_optimal_assignments``, ``permute_blocks`` and ``compute_breakpoint_confidence`` are executed, with stand-ins for
what they import (``it``: itertools; ``log`` / ``exp``: math; ``PhaseBreakpoint``: three attributes).  Nothing of the reference is
written out.

Recorded per case: the inputs (tests/reorder_cases.py generates them), log(1 - error_rate) and log(error_rate) as the recording
interpreter computed them, what the reference's find_breakpoints yields for the threads, and per breakpoint
  - the clusters in the order the reference walked them, read off the read ids handed to extractSubMatrix (clusters of the set without a
    spanning read follow in increasing order: they contribute nothing wherever they stand),
  - the window (left and right positions),
  - every permutation's llh in dict order (checked to be itertools.permutations order),
  - the chosen permutation's rank,
and the assignments, the final threads and haplotypes and the confidences of run_reordering.
No case is dropped.  Breakpoints whose largest llh is shared by several permutations are kept and counted; the generator fails if there
is none.
Usage: python tests/golden/make_reorder_golden.py [/path/to/reference]
       python tests/golden/make_reorder_golden.py /path/to/reference --baseline 40
           (writes nothing: times the reference's own compute_link_likelihoods on the first 40 breakpoints of the benchmark's block, one
           thread -- the figure of profiles/reorder/cpu_baseline.md)
"""
import __future__

import ast
import copy
import ctypes as C
import gzip
import itertools
import json
import math
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "reorder_cases.json.gz")
sys.path.insert(0, os.path.dirname(HERE))
import reorder_cases as rc  # noqa: E402

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
unsigned am_first(void* p, unsigned r) { return ((AlleleMatrix*)p)->getFirstPos(r); }
unsigned am_last(void* p, unsigned r) { return ((AlleleMatrix*)p)->getLastPos(r); }
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
    for name in ("am_first", "am_last"):
        getattr(L, name).restype = C.c_uint
        getattr(L, name).argtypes = [C.c_void_p, C.c_uint]
    L.am_extract.restype = C.c_void_p
    L.am_extract.argtypes = [C.c_void_p, C.POINTER(C.c_uint), C.c_uint, C.POINTER(C.c_uint), C.c_uint, C.c_int]
    L.am_read.restype = C.c_uint
    L.am_read.argtypes = [C.c_void_p, C.c_uint, C.POINTER(C.c_uint), C.POINTER(C.c_int), C.c_uint]
    return L


class RefMatrix:
    """The compiled reference class behind the method names the reference's Python uses; extractSubMatrix notes the read ids it is handed."""

    def __init__(self, L, handle):
        self.L, self.h = L, handle
        self.extract_log = []

    @classmethod
    def from_reads(cls, L, reads):
        read_ptr, pos, alle = [0], [], []
        for row in reads:
            for p, a in row:
                pos.append(rc.global_position(p))
                alle.append(a)
            read_ptr.append(len(pos))
        return cls(L, L.am_new(len(reads), (C.c_ulonglong * len(read_ptr))(*read_ptr), (C.c_int * max(len(pos), 1))(*pos), (C.c_int * max(len(alle), 1))(*alle)))

    def close(self):
        self.L.am_delete(self.h)

    def __len__(self):
        return self.L.am_size(self.h)

    def getNumPositions(self):
        return self.L.am_num_positions(self.h)

    def getFirstPos(self, r):
        return self.L.am_first(self.h, r)

    def getLastPos(self, r):
        return self.L.am_last(self.h, r)

    def getRead(self, r):
        cap = 4096
        pos, alle = (C.c_uint * cap)(), (C.c_int * cap)()
        n = self.L.am_read(self.h, r, pos, alle, cap)
        assert n <= cap
        return [(pos[x], alle[x]) for x in range(n)]

    def __iter__(self):
        return (self.getRead(r) for r in range(len(self)))

    def extractSubMatrix(self, positions, read_ids, remove_empty):
        self.extract_log.append(list(read_ids))
        return RefMatrix(self.L, self.L.am_extract(self.h, (C.c_uint * max(len(positions), 1))(*positions), len(positions),
                                                   (C.c_uint * max(len(read_ids), 1))(*read_ids), len(read_ids), 1 if remove_empty else 0))


class PhaseBreakpoint:
    def __init__(self, position, haplotypes, confidence):
        self.position = position
        self.haplotypes = sorted(haplotypes[:])
        self.confidence = confidence


WANTED = ("run_reordering", "compute_link_likelihoods", "get_heterozygous_pos_for_haps", "find_breakpoints", "get_optimal_assignments", "permute_blocks",
          "compute_breakpoint_confidence")


def load_reference_functions(ref_root):
    """The seven functions of the reference's reorder.py, compiled from its own text at run time (annotations are not evaluated)."""
    path = os.path.join(ref_root, "whatshap", "polyphase", "reorder.py")
    tree = ast.parse(open(path).read(), filename=path)
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in WANTED]
    assert sorted(n.name for n in keep) == sorted(WANTED)
    ns = {"it": itertools, "log": math.log, "exp": math.exp, "PhaseBreakpoint": PhaseBreakpoint}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec", flags=__future__.annotations.compiler_flag), ns)
    return ns


def record_case(L, ns, case):
    am = RefMatrix.from_reads(L, case["reads"])
    assert am.getNumPositions() == case["n_pos"]
    threads, haps, clustering, err = case["threads"], case["haplotypes"], case["clustering"], case["error_rate"]
    cluster_of = {r: c for c, members in enumerate(clustering) for r in members}
    bps = [PhaseBreakpoint(pos, affected, 0.0) for pos, affected in case["breakpoints"]]
    rec = dict(case)
    rec["log_match"], rec["log_err"] = math.log(1 - err).hex(), math.log(err).hex()
    found = ns["find_breakpoints"](threads)
    rec["ref_find_breakpoints"] = [[b.position, list(b.haplotypes)] for b in found]
    assert rec["ref_find_breakpoints"] == rc.find_breakpoints(threads)
    lllh = ns["compute_link_likelihoods"](threads, haps, bps, clustering, am, err)
    assert len(am.extract_log) == len(bps)
    expected, ties = [], 0
    for b, d in zip(bps, lllh):
        pos, affected = b.position, b.haplotypes
        assert list(d.keys()) == list(itertools.permutations(affected))
        walked = []
        for r in am.extract_log[len(expected)]:
            if cluster_of[r] not in walked:
                walked.append(cluster_of[r])
        in_set = {threads[pos][h] for h in affected} | {threads[pos - 1][h] for h in affected}
        assert set(walked) <= in_set
        walked += sorted(in_set - set(walked))
        left, right = ns["get_heterozygous_pos_for_haps"](haps, affected, pos, 32)
        values = list(d.values())
        chosen = max(d, key=d.get)
        ties += values.count(max(values)) > 1
        expected.append(dict(clusters=[int(c) for c in walked], left=[int(p) for p in left], right=[int(p) for p in right],
                             llh=[float(v).hex() for v in values], chosen=list(d.keys()).index(chosen)))
    rec["expected"] = expected
    rec["assignments"] = [[int(x) for x in a] for a in ns["get_optimal_assignments"](bps, lllh, case["ploidy"], None)]
    threads2, haps2 = copy.deepcopy(threads), copy.deepcopy(haps)
    ns["run_reordering"](am, clustering, threads2, haps2, bps, None, err)
    rec["final_threads"], rec["final_haplotypes"] = threads2, haps2
    rec["confidence"] = [float(b.confidence).hex() for b in bps]
    am.close()
    return rec, ties


def baseline(ref_root, n_breakpoints):
    """The reference's compute_link_likelihoods on the compiled matrix: the first n_breakpoints breakpoints of rc.large_problem()."""
    import time

    ns = load_reference_functions(ref_root)
    case = rc.large_problem()
    bps = [PhaseBreakpoint(pos, affected, 0.0) for pos, affected in case["breakpoints"]]
    with tempfile.TemporaryDirectory() as tmp:
        L = build_wrapper(ref_root, tmp)
        am = RefMatrix.from_reads(L, case["reads"])
        t0 = time.perf_counter()
        lllh = ns["compute_link_likelihoods"](case["threads"], case["haplotypes"], bps[:n_breakpoints], case["clustering"], am, case["error_rate"])
        t1 = time.perf_counter()
    print(json.dumps({"positions": case["n_pos"], "reads": len(case["reads"]), "breakpoints_total": len(bps), "breakpoints_timed": len(lllh),
                      "permutations_timed": sum(len(d) for d in lllh), "permutations_total": sum(math.factorial(len(b.haplotypes)) for b in bps),
                      "compute_link_likelihoods_s": round(t1 - t0, 3)}))


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("WHATSHAP_REFERENCE", "")
    if not ref_root or not os.path.isdir(os.path.join(ref_root, "src", "polyphase")):
        sys.exit("usage: make_reorder_golden.py /path/to/reference (a WhatsHap source tree)")
    if len(sys.argv) > 3 and sys.argv[2] == "--baseline":
        return baseline(ref_root, int(sys.argv[3]))
    ns = load_reference_functions(ref_root)
    with tempfile.TemporaryDirectory() as tmp:
        L = build_wrapper(ref_root, tmp)
        recorded = [record_case(L, ns, case) for case in rc.all_cases()]
    cases, ties = [r[0] for r in recorded], sum(r[1] for r in recorded)
    assert ties > 0, "no breakpoint with a tied best permutation was recorded"
    with gzip.GzipFile(OUT, "wb", mtime=0) as f:
        f.write(json.dumps({"cases": cases, "tied_breakpoints": ties}, separators=(",", ":")).encode())
    print(f"{len(cases)} cases, {sum(len(c['expected']) for c in cases)} breakpoints ({ties} with a tied best permutation), "
          f"{sum(len(e['llh']) for c in cases for e in c['expected'])} llh values -> {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
