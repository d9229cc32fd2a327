#!/usr/bin/env python3
"""Writes tests/golden/compare_cases.json.gz: what the reference's polyploid phasing comparison returns for the cases of
tests/compare_cases.py (run only where the reference tree exists; the tests read the recorded data).

The reference's src/polyphase/switchflipcalculator.cpp is compiled with a small extern "C" wrapper (written here, below) into a temporary
directory outside the repository and loaded with ctypes: SwitchFlipCalculator::compare is the reference's own.  The reference's own Python
functions run against it: at generation time whatshap/cli/compare.py is parsed and only ``SwitchFlips``, ``PhasingErrors``, ``hamming``,
``switch_encoding``, ``compute_switch_flips``, ``compute_matching_genotype_pos``, ``compute_switch_errors_poly``,
``compute_switch_flips_poly``, ``compute_switch_flips_poly_bt`` and ``compare_block`` are executed, with stand-ins for what they import
(``Genotype``: the sorted alleles; ``SwitchFlipCalculator``: the Cython class's one method over the compiled calculator; ``permutations``,
``Optional``, ``logger``).  Nothing of the reference is written out.

Recorded per case: the inputs (tests/compare_cases.py generates them), the fields of compare_block's PhasingErrors, the matching
positions, compute_switch_errors_poly, and per cost pair what compute_switch_flips_poly_bt returns: the raw (switches, flips) -- the
returned fractions times the ploidy -- and the three per-column lists.
No case is dropped.  The generator fails if a recorded case has fewer reference flips than compare_cases.dense_oracle, if a total differs
from dense_oracle's, or if no recorded split differs from the canonical one: the set must show that the tie rule matters.
Usage: python tests/golden/make_compare_golden.py [/path/to/reference]
       python tests/golden/make_compare_golden.py /path/to/reference --baseline 20
           (writes nothing: times the reference's own compare_block on the first 20 blocks of the benchmark, one thread -- the figure
           of profiles/compare/cpu_baseline.md)
"""
import __future__

import ast
import ctypes as C
import gzip
import itertools
import json
import logging
import os
import subprocess
import sys
import tempfile
from typing import Optional

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "compare_cases.json.gz")
sys.path.insert(0, os.path.dirname(HERE))
import compare_cases as cc  # noqa: E402

WRAPPER = r"""
#include <cstdint>
#include <vector>
#include "polyphase/switchflipcalculator.h"
extern "C" int sfc_compare(unsigned ploidy, double switch_cost, double flip_cost, unsigned n, const unsigned* p0, const unsigned* p1, double* result,
                           unsigned* switches_out, int* flipped_out, unsigned* perm_out) {
    std::vector<std::vector<uint32_t>> a(n), b(n), flipped, perm;
    std::vector<uint32_t> switches;
    for (unsigned x = 0; x < n; x++) {
        a[x].assign(p0 + x * ploidy, p0 + (x + 1) * ploidy);
        b[x].assign(p1 + x * ploidy, p1 + (x + 1) * ploidy);
    }
    SwitchFlipCalculator calc(ploidy, switch_cost, flip_cost);
    std::pair<double, double> r = calc.compare(a, b, switches, flipped, perm);
    result[0] = r.first;
    result[1] = r.second;
    if (switches.size() != n || flipped.size() != n || perm.size() != n) return 0;
    for (unsigned x = 0; x < n; x++) {
        switches_out[x] = switches[x];
        for (unsigned i = 0; i < ploidy; i++) {
            flipped_out[x * ploidy + i] = i < flipped[x].size() ? (int)flipped[x][i] : -1;
            perm_out[x * ploidy + i] = perm[x][i];
        }
    }
    return 1;
}
"""


def build_wrapper(ref_root, tmp):
    src = os.path.join(tmp, "wrapper.cpp")
    open(src, "w").write(WRAPPER)
    so = os.path.join(tmp, "libsfc.so")
    srcdir = os.path.join(ref_root, "src")
    subprocess.run(["g++", "-O2", "-std=c++14", "-shared", "-fPIC", "-I" + srcdir, "-I" + os.path.join(srcdir, "polyphase"), src,
                    os.path.join(srcdir, "polyphase", "switchflipcalculator.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    L.sfc_compare.restype = C.c_int
    L.sfc_compare.argtypes = [C.c_uint, C.c_double, C.c_double, C.c_uint, C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(C.c_double),
                              C.POINTER(C.c_uint), C.POINTER(C.c_int), C.POINTER(C.c_uint)]
    return L


class Genotype:
    """whatshap.core.Genotype as far as compute_matching_genotype_pos uses it: the multiset of alleles."""

    def __init__(self, alleles):
        self.alleles = sorted(alleles)

    def __eq__(self, other):
        return self.alleles == other.alleles


def calculator_class(L):
    class SwitchFlipCalculator:
        """The Cython class of whatshap/polyphase/solver.pyx over the compiled calculator: the same conversion of haplotype-wise strings to
        position-wise ints, the same five return values."""

        def __init__(self, ploidy, switch_cost=1, flip_cost=1):
            self.ploidy, self.switch_cost, self.flip_cost = ploidy, switch_cost, flip_cost

        def compute_switch_flips_poly(self, phasing0, phasing1):
            assert len(phasing0) == len(phasing1) == self.ploidy
            assert self.ploidy >= 2
            assert len(phasing0[0]) > 0
            k, n = self.ploidy, len(phasing0[0])
            flat0 = [int(phasing0[h][i]) for i in range(n) for h in range(k)]
            flat1 = [int(phasing1[h][i]) for i in range(n) for h in range(k)]
            result = (C.c_double * 2)()
            switches, flipped, perm = (C.c_uint * n)(), (C.c_int * (n * k))(), (C.c_uint * (n * k))()
            have = L.sfc_compare(k, self.switch_cost, self.flip_cost, n, (C.c_uint * len(flat0))(*flat0), (C.c_uint * len(flat1))(*flat1), result,
                                 switches, flipped, perm)
            if not have:
                return result[0], result[1], [], [], []
            return (result[0], result[1], list(switches), [[f for f in flipped[x * k:(x + 1) * k] if f >= 0] for x in range(n)],
                    [list(perm[x * k:(x + 1) * k]) for x in range(n)])

    return SwitchFlipCalculator


WANTED = ("SwitchFlips", "PhasingErrors", "hamming", "switch_encoding", "compute_switch_flips", "compute_matching_genotype_pos", "compute_switch_errors_poly",
          "compute_switch_flips_poly", "compute_switch_flips_poly_bt", "compare_block")


def load_reference_functions(ref_root, L):
    """The classes and functions of the reference's compare.py listed above, compiled from its own text at run time."""
    path = os.path.join(ref_root, "whatshap", "cli", "compare.py")
    tree = ast.parse(open(path).read(), filename=path)
    keep = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in WANTED]
    assert sorted(n.name for n in keep) == sorted(WANTED)
    ns = {"permutations": itertools.permutations, "Optional": Optional, "logger": logging.getLogger("reference.compare"), "Genotype": Genotype,
          "SwitchFlipCalculator": calculator_class(L)}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec", flags=__future__.annotations.compiler_flag), ns)
    return ns


def record_case(ns, case):
    p0, p1 = cc.arrays(case)
    n_pos, k = p0.shape
    s0, s1 = case["phasing0"], case["phasing1"]
    block = ns["compare_block"](s0, s1)
    ref = dict(block=dict(switches=block.switches, hamming=block.hamming, switch_flips=[block.switch_flips.switches, block.switch_flips.flips],
                          diff_genotypes=block.diff_genotypes),
               matching_pos=[int(x) for x in ns["compute_matching_genotype_pos"](s0, s1)], switch_errors=ns["compute_switch_errors_poly"](s0, s1), runs=[])
    differs = 0
    for sc, fc in case["costs"]:
        result, switches_in_column, flips_in_column, config = ns["compute_switch_flips_poly_bt"](s0, s1, switch_cost=sc, flip_cost=fc)
        raw = [round(result.switches * k), round(result.flips * k)]
        assert raw[0] / k == result.switches and raw[1] / k == result.flips
        assert raw == [sum(switches_in_column), sum(len(f) for f in flips_in_column)]
        ref["runs"].append(dict(raw=raw, switches_in_column=switches_in_column, flips_in_column=flips_in_column, config=config))
        if n_pos > 1:
            total, switches, flips = cc.dense_oracle(p0, p1, sc, fc)
            assert sc * raw[0] + fc * raw[1] == total, (case["name"], sc, fc, raw, total)
            assert raw[1] >= flips, (case["name"], sc, fc, raw, flips)
            differs += raw != [switches, flips]
    rec = dict(case)
    rec["ref"] = ref
    return rec, differs


def baseline(ref_root, n_blocks):
    """The reference's compare_block over the compiled calculator on the first n_blocks blocks of the benchmark, and on its long block."""
    import time

    with tempfile.TemporaryDirectory() as tmp:
        ns = load_reference_functions(ref_root, build_wrapper(ref_root, tmp))
        blocks = []
        for seed in range(n_blocks):
            p0, p1 = cc.bench_block(seed)
            blocks.append((cc._strings(p0.tolist()), cc._strings(p1.tolist())))
        t0 = time.perf_counter()
        for s0, s1 in blocks:
            ns["compare_block"](s0, s1)
        t1 = time.perf_counter()
        out = {"ploidy": 6, "positions": 500, "blocks_timed": n_blocks, "compare_block_s": round(t1 - t0, 3)}
        p0, p1 = cc.bench_block(12345, n_pos=100000)
        s0, s1 = cc._strings(p0.tolist()), cc._strings(p1.tolist())
        t0 = time.perf_counter()
        ns["compare_block"](s0, s1)
        out["long_block_positions"], out["long_block_compare_block_s"] = 100000, round(time.perf_counter() - t0, 3)
    print(json.dumps(out))


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("WHATSHAP_REFERENCE", "")
    if not ref_root or not os.path.isdir(os.path.join(ref_root, "src", "polyphase")):
        sys.exit("usage: make_compare_golden.py /path/to/reference (a WhatsHap source tree)")
    if len(sys.argv) > 3 and sys.argv[2] == "--baseline":
        return baseline(ref_root, int(sys.argv[3]))
    with tempfile.TemporaryDirectory() as tmp:
        ns = load_reference_functions(ref_root, build_wrapper(ref_root, tmp))
        recorded = [record_case(ns, case) for case in cc.all_cases()]
    cases, differs = [r[0] for r in recorded], sum(r[1] for r in recorded)
    assert differs > 0, "no recorded split differs from the canonical one"
    with gzip.GzipFile(OUT, "wb", mtime=0) as f:
        f.write(json.dumps({"cases": cases, "splits_that_differ": differs}, separators=(",", ":")).encode())
    print(f"{len(cases)} cases, {sum(len(c['ref']['runs']) for c in cases)} runs ({differs} with a reference split other than the canonical one) -> {OUT} "
          f"({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
