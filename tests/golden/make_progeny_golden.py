#!/usr/bin/env python3
"""Writes tests/golden/progeny_cases.json.gz: what the reference's progeny marker scoring returns for the cases of tests/progeny_cases.py
(run only where the reference tree exists; the tests read the recorded data).

The reference's src/polyphase/progenygenotypelikelihoods.cpp is compiled with a small extern "C" wrapper (written here, below) into a
temporary directory outside the repository and loaded with ctypes.  The reference's own Python functions run against it: at generation
time whatshap/polyphase/offspringscoring.py is parsed and only ``hyp``, ``compute_gt_likelihood_priors``, ``get_most_likely_variant_type``
and ``get_variant_scoring`` are executed, with stand-ins for what they import (``TriangleSparseMatrix``: a dict that rounds to float as
the reference's set does; ``binom_coeff``: scipy.special.binom; ``log`` / ``isnan``: math).  Nothing of the reference is written out.

Recorded per pair-score case: the spec (tests/progeny_cases.py generates the inputs from it), the SHA-256 of the generated table, the
exception class where the reference raises, else every stored entry in triangular order -- (i, j), the double score's bits, the float
score's bits -- and a SHA-256 over the complete list; for the medium case the digest and every 75th entry only (file size).  Also a
sample of the class's getters and single-pair scores, rows set beyond numPositions included.
Recorded for the variant types: compute_gt_likelihood_priors for ploidy 2 .. 12, and per case the winner of every variant and the
reference's llh of every parental type (read from the running function's frame at its comparison ``llh > best_llh``).  The generator
fails -- it drops nothing -- if in any recorded variant the best and the second-best llh differ by 1e-6 or less.
Usage: python tests/golden/make_progeny_golden.py [/path/to/reference]
       python tests/golden/make_progeny_golden.py /path/to/reference --baseline 2000
           (writes nothing: times the reference's own loop on the first 2 000 nodes of the benchmark's problem, one thread --
           the figure of profiles/progeny/cpu_baseline.md)
"""
import ast
import ctypes as C
import gzip
import json
import math
import os
import random
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "progeny_cases.json.gz")
sys.path.insert(0, os.path.dirname(HERE))
import progeny_cases as pc  # noqa: E402

WRAPPER = r"""
#include <cstddef>
#include <sys/types.h>
#include <vector>
#include "polyphase/progenygenotypelikelihoods.h"
extern "C" {
void* pgl_new(unsigned ploidy, unsigned n_samples, unsigned n_positions) { return new ProgenyGenotypeLikelihoods(ploidy, n_samples, n_positions); }
void pgl_delete(void* p) { delete (ProgenyGenotypeLikelihoods*)p; }
double pgl_get_gl(void* p, unsigned pos, unsigned s, unsigned g) { return ((ProgenyGenotypeLikelihoods*)p)->getGl(pos, s, g); }
void pgl_get_glv(void* p, unsigned pos, unsigned s, double* out) {
    std::vector<double> v = ((ProgenyGenotypeLikelihoods*)p)->getGlv(pos, s);
    for (std::size_t i = 0; i < v.size(); i++) out[i] = v[i];
}
void pgl_set_gl(void* p, unsigned pos, unsigned s, unsigned g, double l) { ((ProgenyGenotypeLikelihoods*)p)->setGl(pos, s, g, l); }
void pgl_set_glv(void* p, unsigned pos, unsigned s, const double* l, unsigned n) {
    ((ProgenyGenotypeLikelihoods*)p)->setGlv(pos, s, std::vector<double>(l, l + n));
}
unsigned pgl_ploidy(void* p) { return ((ProgenyGenotypeLikelihoods*)p)->getPloidy(); }
unsigned pgl_samples(void* p) { return ((ProgenyGenotypeLikelihoods*)p)->getNumSamples(); }
unsigned pgl_positions(void* p) { return ((ProgenyGenotypeLikelihoods*)p)->getNumPositions(); }
double pgl_sn(void* p, unsigned a, unsigned b) { return ((ProgenyGenotypeLikelihoods*)p)->getSimplexNulliplexScore(a, b); }
double pgl_s2(void* p, unsigned a, unsigned b) { return ((ProgenyGenotypeLikelihoods*)p)->getSimplexSimplexScore(a, b); }
double pgl_dn(void* p, unsigned a, unsigned b) { return ((ProgenyGenotypeLikelihoods*)p)->getDuplexNulliplexScore(a, b); }
}
"""


def build_wrapper(ref_root, tmp):
    src = os.path.join(tmp, "wrapper.cpp")
    open(src, "w").write(WRAPPER)
    so = os.path.join(tmp, "libpgl.so")
    srcdir = os.path.join(ref_root, "src")
    subprocess.run(["g++", "-O2", "-std=c++14", "-shared", "-fPIC", "-I" + srcdir, src, os.path.join(srcdir, "polyphase", "progenygenotypelikelihoods.cpp"),
                    "-o", so], check=True)
    L = C.CDLL(so)
    L.pgl_new.restype = C.c_void_p
    L.pgl_new.argtypes = [C.c_uint, C.c_uint, C.c_uint]
    L.pgl_delete.argtypes = [C.c_void_p]
    L.pgl_get_gl.restype = C.c_double
    L.pgl_get_gl.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_uint]
    L.pgl_get_glv.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.POINTER(C.c_double)]
    L.pgl_set_gl.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_double]
    L.pgl_set_glv.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.POINTER(C.c_double), C.c_uint]
    for name in ("pgl_ploidy", "pgl_samples", "pgl_positions"):
        getattr(L, name).restype = C.c_uint
        getattr(L, name).argtypes = [C.c_void_p]
    for name in ("pgl_sn", "pgl_s2", "pgl_dn"):
        getattr(L, name).restype = C.c_double
        getattr(L, name).argtypes = [C.c_void_p, C.c_uint, C.c_uint]
    return L


class RefTable:
    """The compiled reference class behind the method names the reference's Python uses."""

    def __init__(self, L, ploidy, n_samples, n_positions):
        self.L, self.h = L, L.pgl_new(ploidy, n_samples, n_positions)

    def close(self):
        self.L.pgl_delete(self.h)

    def getGl(self, pos, s, g):
        return self.L.pgl_get_gl(self.h, pos, s, g)

    def getGlv(self, pos, s):
        out = (C.c_double * (self.getPloidy() + 1))()
        self.L.pgl_get_glv(self.h, pos, s, out)
        return list(out)

    def setGl(self, pos, s, g, l):
        self.L.pgl_set_gl(self.h, pos, s, g, l)

    def setGlv(self, pos, s, l):
        self.L.pgl_set_glv(self.h, pos, s, (C.c_double * len(l))(*l), len(l))

    def getPloidy(self):
        return self.L.pgl_ploidy(self.h)

    def getNumSamples(self):
        return self.L.pgl_samples(self.h)

    def getNumPositions(self):
        return self.L.pgl_positions(self.h)

    def getSimplexNulliplexScore(self, a, b):
        return self.L.pgl_sn(self.h, a, b)

    def getSimplexSimplexScore(self, a, b):
        return self.L.pgl_s2(self.h, a, b)

    def getDuplexNulliplexScore(self, a, b):
        return self.L.pgl_dn(self.h, a, b)

    def fill(self, table):
        for pos in range(table.shape[0]):
            for s in range(table.shape[1]):
                if table[pos, s, 0] >= 0:
                    self.setGlv(pos, s, [float(x) for x in table[pos, s]])


class RecordingMatrix:
    """Stand-in for TriangleSparseMatrix: set(i, j, score) keeps the double and the float it is stored as."""

    def __init__(self):
        self.m = {}

    def set(self, i, j, score):
        if i != j:
            self.m[(max(i, j), min(i, j))] = float(score)


WANTED = ("hyp", "compute_gt_likelihood_priors", "get_most_likely_variant_type", "get_variant_scoring")


def load_reference_functions(ref_root):
    """The four functions of the reference's offspringscoring.py, compiled from its own text at run time, and the line of
    get_most_likely_variant_type's comparison ``llh > best_llh``."""
    from scipy.special import binom as binom_coeff

    path = os.path.join(ref_root, "whatshap", "polyphase", "offspringscoring.py")
    tree = ast.parse(open(path).read(), filename=path)
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in WANTED]
    assert sorted(n.name for n in keep) == sorted(WANTED)
    for n in keep:
        n.decorator_list = []
    ns = {"TriangleSparseMatrix": RecordingMatrix, "binom_coeff": binom_coeff, "log": math.log, "isnan": math.isnan}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    fn = next(n for n in keep if n.name == "get_most_likely_variant_type")
    compare = [n for n in ast.walk(fn) if isinstance(n, ast.If) and isinstance(n.test, ast.Compare) and getattr(n.test.left, "id", "") == "llh"
               and getattr(n.test.comparators[0], "id", "") == "best_llh"]
    assert len(compare) == 1
    return ns, compare[0].lineno


def all_type_llh(ns, compare_line, priors, table, pos):
    """get_most_likely_variant_type(priors, None, table, pos) -> (winner, [llh of every type in loop order]) -- the llh values are the
    running function's own, read at its comparison."""
    seen = []

    def tracer(frame, event, arg):
        if frame.f_code.co_name != "get_most_likely_variant_type":
            return None
        if event == "line" and frame.f_lineno == compare_line:
            seen.append(frame.f_locals["llh"])
        return tracer

    sys.settrace(tracer)
    try:
        winner = ns["get_most_likely_variant_type"](priors, None, table, pos)
    finally:
        sys.settrace(None)
    return winner, seen


def hexes(values):
    return [float(v).hex() for v in values]


def record_pair_case(L, ns, spec):
    table, node_variant, alt, co = pc.build_pair_case(spec)
    rec = dict(spec=spec, table_sha256=pc.table_sha256(table), n_positions=int(table.shape[0]), n_nodes=int(node_variant.size))
    ref = RefTable(L, spec["ploidy"], spec["n_samples"], table.shape[0])
    rng = random.Random(spec["seed"] + 999)
    try:
        ref.fill(table)
        beyond = []
        for x in range(spec["rows_beyond"]):   # rows set beyond numPositions: the vector grows, numPositions does not
            pos, s = table.shape[0] + x, rng.randrange(spec["n_samples"])
            row = [rng.random() for _ in range(spec["ploidy"] + 1)]
            ref.setGlv(pos, s, row)
            ref.setGl(pos, s, 0, 0.25)
            beyond.append(dict(pos=pos, sample=s, row=hexes(row)))
        rec["set_beyond"] = beyond
        rec["num_positions_after"] = ref.getNumPositions()
        # getters
        gets = []
        if spec["n_samples"] and node_variant.size:
            for _ in range(8):
                pos, s, g = rng.randrange(node_variant.size + 2), rng.randrange(spec["n_samples"]), rng.randrange(spec["ploidy"] + 1)
                gets.append(dict(pos=pos, sample=s, genotype=g, gl=float(ref.getGl(pos, s, g)).hex(), glv=hexes(ref.getGlv(pos, s))))
        rec["getters"] = gets
        pairs = []
        if node_variant.size >= 2:
            for _ in range(9):
                a, b = rng.randrange(node_variant.size), rng.randrange(node_variant.size)
                pairs.append(dict(pos1=a, pos2=b, sn=float(ref.getSimplexNulliplexScore(a, b)).hex(), s2=float(ref.getSimplexSimplexScore(a, b)).hex(),
                                  dn=float(ref.getDuplexNulliplexScore(a, b)).hex()))
        rec["pair_scores"] = pairs
        try:
            scoring = ns["get_variant_scoring"](pc.VarInfo(node_variant, alt, co), ref, pc.Param(spec["window"]))
        except Exception as e:   # (windows below 4: IndexError from the stride list)
            rec["raises"] = type(e).__name__
            return rec
    finally:
        ref.close()
    keys = sorted(scoring.m)
    hi = np.array([k[0] for k in keys], dtype=np.uint32)
    lo = np.array([k[1] for k in keys], dtype=np.uint32)
    f64 = np.array([scoring.m[k] for k in keys], dtype=np.float64)
    with np.errstate(over="ignore"):
        f32_bits = f64.astype(np.float32).view(np.uint32)
    rec["n_entries"] = len(keys)
    rec["digest"] = pc.entries_digest(hi, lo, f64, f32_bits)
    step = 75 if spec["name"] == "medium" else 1
    rec["step"] = step
    rec["i"] = pc.pack(hi[::step], "<u4")
    rec["j"] = pc.pack(lo[::step], "<u4")
    rec["f64"] = pc.pack(f64[::step], "<f8")
    rec["f32_bits"] = pc.pack(f32_bits[::step], "<u4")
    return rec


def record_type_case(L, ns, compare_line, spec):
    priors = ns["compute_gt_likelihood_priors"](spec["ploidy"])
    priors = [[[float(x) for x in d] for d in row] for row in priors]
    table, truth = pc.build_type_case(spec, priors)
    ref = RefTable(L, spec["ploidy"], spec["n_samples"], table.shape[0])
    try:
        ref.fill(table)
        winners, llh = [], []
        for pos in range(table.shape[0]):
            w, values = all_type_llh(ns, compare_line, priors, ref, pos)
            assert len(values) == (spec["ploidy"] + 1) * (spec["ploidy"] + 2) // 2
            ordered = sorted(values, reverse=True)
            margin = ordered[0] - ordered[1]
            assert margin > 1e-6, f"{spec['name']} variant {pos}: best and second-best llh differ by {margin}"
            winners.append([int(w[0]), int(w[1])])
            llh.append(values)
    finally:
        ref.close()
    return dict(spec=spec, table_sha256=pc.table_sha256(table), truth=[list(t) for t in truth], winners=winners,
                llh=pc.pack(np.array(llh, dtype=np.float64), "<f8"))


def baseline(ref_root, n_nodes):
    """The reference's get_variant_scoring on the compiled class: the first n_nodes nodes of progeny_cases.large_problem()."""
    import time

    ns, _ = load_reference_functions(ref_root)
    table, node_variant, alt, co, window = pc.large_problem()
    table, node_variant = table[:n_nodes], node_variant[:n_nodes]
    with tempfile.TemporaryDirectory() as tmp:
        L = build_wrapper(ref_root, tmp)
        ref = RefTable(L, 4, table.shape[1], n_nodes)
        t0 = time.perf_counter()
        ref.fill(table)
        t1 = time.perf_counter()
        scoring = ns["get_variant_scoring"](pc.VarInfo(node_variant, alt, co), ref, pc.Param(window))
        t2 = time.perf_counter()
        ref.close()
    n_inf = sum(1 for v in scoring.m.values() if v == -math.inf)
    terms = (len(scoring.m) - n_inf) * table.shape[1]
    print(json.dumps({"nodes": n_nodes, "samples": int(table.shape[1]), "window": window, "entries": len(scoring.m), "sample_terms": terms,
                      "fill_table_s": round(t1 - t0, 3), "get_variant_scoring_s": round(t2 - t1, 3), "entries_per_s": len(scoring.m) / (t2 - t1),
                      "sample_terms_per_s": terms / (t2 - t1)}))


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("WHATSHAP_REFERENCE", "")
    if not ref_root or not os.path.isdir(os.path.join(ref_root, "src", "polyphase")):
        sys.exit("usage: make_progeny_golden.py /path/to/reference (a WhatsHap source tree)")
    if len(sys.argv) > 3 and sys.argv[2] == "--baseline":
        return baseline(ref_root, int(sys.argv[3]))
    ns, compare_line = load_reference_functions(ref_root)
    with tempfile.TemporaryDirectory() as tmp:
        L = build_wrapper(ref_root, tmp)
        pairs = [record_pair_case(L, ns, spec) for spec in pc.pair_specs()]
        types = [record_type_case(L, ns, compare_line, spec) for spec in pc.type_specs()]
    priors = {str(k): [[hexes(d) for d in row] for row in ns["compute_gt_likelihood_priors"](k)] for k in range(2, 13)}
    with gzip.GzipFile(OUT, "wb", mtime=0) as f:
        f.write(json.dumps({"pair_cases": pairs, "type_cases": types, "priors": priors}, separators=(",", ":")).encode())
    print(f"{len(pairs)} pair cases ({sum(c.get('n_entries', 0) for c in pairs)} entries, {sum(1 for c in pairs if 'raises' in c)} raise), "
          f"{len(types)} type cases ({sum(len(c['winners']) for c in types)} variants) -> {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
