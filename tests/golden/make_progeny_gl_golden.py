#!/usr/bin/env python3
"""Writes tests/golden/progeny_gl_cases.json.gz: what the reference's get_offspring_gl, compute_gt_likelihoods and correct_variant_types
return for the cases of tests/progeny_gl_cases.py (run only where the reference tree exists; the tests read the recorded data).

As make_progeny_golden.py does, the reference's src/polyphase/progenygenotypelikelihoods.cpp is compiled with that file's small wrapper
into a temporary directory and loaded with ctypes, and the reference's own Python runs against it: at generation time
whatshap/polyphase/offspringscoring.py and variantselection.py are parsed and only ``get_binom_pmf``, ``hyp``,
``compute_gt_likelihood_priors``, ``compute_gt_likelihoods``, ``get_offspring_gl``, ``correct_variant_types``,
``get_most_likely_variant_type`` and the class ``VariantInfo`` are executed, with stand-ins for what they import (``binom``: scipy.stats;
``ProgenyGenotypeLikelihoods``: the compiled class; the variant tables: tests/progeny_gl_cases.Table).  Nothing of the reference is
written out.

Recorded per case: the spec (tests/progeny_gl_cases.py generates the inputs from it) and the SHA-256 of the generated inputs; what
get_offspring_gl leaves in the VariantInfo (phasable set, types) and the nodes it makes; the reference's doubles -- compute_gt_likelihoods
per sample with the priors, [node][sample][genotype], -1 where it returns None -- as bits; the float table of the compiled class after
get_offspring_gl as bits; compute_gt_likelihoods without priors for the first sample; and the VariantInfo state correct_variant_types leaves.
Recorded once: what the reference does at the deep cells progeny_gl_cases.UNDERFLOWING (its normalising sum, and whether it raises or
returns NaN); E_ref, the largest relative deviation of the reference's doubles from the exact rational values
(progeny_gl_cases.exact_cell), and the smallest normalising sum the reference formed.
The generator fails -- it drops nothing -- if a normalising sum is not above 1e-280, or if a recorded double lies closer to a float
rounding boundary than 10 * E_ref relative (change that case's seed and run again).
Usage: python tests/golden/make_progeny_gl_golden.py /path/to/reference
       python tests/golden/make_progeny_gl_golden.py /path/to/reference --baseline 300
           (writes nothing: times the reference's own get_offspring_gl on the first 300 nodes of the benchmark's depth problem, one
           thread -- the figure of profiles/progeny/cpu_baseline.md)
"""
import ast
import collections
import functools
import gzip
import json
import logging
import math
import os
import sys
import tempfile
import typing
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "progeny_gl_cases.json.gz")
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_progeny_golden as base  # noqa: E402
import progeny_gl_cases as gc  # noqa: E402

WANTED = ("get_binom_pmf", "hyp", "compute_gt_likelihood_priors", "compute_gt_likelihoods", "get_offspring_gl", "correct_variant_types",
          "get_most_likely_variant_type")


def load_reference(ref_root, L):
    """The namespace with the reference's functions and its VariantInfo, compiled from its own text at run time."""
    from scipy.special import binom as binom_coeff
    from scipy.stats import binom

    path = os.path.join(ref_root, "whatshap", "polyphase", "variantselection.py")
    tree = ast.parse(open(path).read(), filename=path)
    keep = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "VariantInfo"]
    assert len(keep) == 1
    ns = {"List": typing.List, "VariantTable": object, "logger": logging.getLogger("reference")}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    path = os.path.join(ref_root, "whatshap", "polyphase", "offspringscoring.py")
    tree = ast.parse(open(path).read(), filename=path)
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in WANTED]
    assert sorted(n.name for n in keep) == sorted(WANTED)
    ns.update({"binom": binom, "binom_coeff": binom_coeff, "lru_cache": functools.lru_cache, "log": math.log, "isnan": math.isnan,
               "defaultdict": collections.defaultdict, "Iterable": typing.Iterable, "Tuple": typing.Tuple,
               "ProgenyGenotypeLikelihoods": lambda ploidy, n_samples, n_positions: base.RefTable(L, ploidy, n_samples, n_positions)})
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns


def boundary_distance(v):
    """The relative distance of the double v > 0 from the nearest value at which its float rounding changes."""
    f = np.float32(v)
    mids = [(float(f) + float(np.nextafter(f, np.float32(x)))) / 2 for x in (np.inf, -np.inf)]
    return min(abs(v - m) for m in mids) / v


def record_case(ns, spec, totals):
    case = gc.Case(spec)
    k = spec["ploidy"]
    rec = dict(spec=spec, inputs_sha256=case.sha256())
    info = case.varinfo(ns["VariantInfo"])
    off_gl = ns["get_offspring_gl"](case.variant_table, case.progeny_table, case.offspring, info, case.param)
    try:
        nodes = info.get_node_positions()
        assert off_gl.getNumPositions() == len(nodes)
        rec["after_gl"] = gc.state_of(info)
        rec["nodes"] = nodes
        f32 = np.array([[off_gl.getGlv(n, s) for s in range(len(case.offspring))] for n in range(len(nodes))], dtype=np.float64).reshape(
            len(nodes), len(case.offspring), k + 1)
        assert np.array_equal(f32.astype(np.float32).astype(np.float64), f32)
        rec["f32_bits"] = gc.pack(f32.astype(np.float32).view(np.uint32), "<u4")
    finally:
        off_gl.close()
    # the doubles: compute_gt_likelihoods as get_offspring_gl calls it, and the progeny positions it pairs the nodes with
    progeny_pos = {}
    for i in range(len(case.progeny_table)):
        if case.progeny_table.variants[i].position:
            progeny_pos[case.progeny_table.variants[i].position] = i
    pairs = [(v, progeny_pos[case.variant_table.variants[v].position]) for v in nodes]
    priors = ns["compute_gt_likelihood_priors"](k)
    f64 = np.full((len(nodes), len(case.offspring), k + 1), -1.0)
    for s, sample in enumerate(case.offspring):
        for n, gl in enumerate(ns["compute_gt_likelihoods"](case.progeny_table, sample, pairs, info, case.param, priors)):
            if gl:
                f64[n, s] = gl
    with np.errstate(under="ignore"):
        assert np.array_equal(f64.astype(np.float32).view(np.uint32), gc.unpack(rec["f32_bits"], "<u4").reshape(f64.shape)), "setGlv does not round the doubles?"
    rec["f64"] = gc.pack(f64, "<f8")
    plain = np.full((len(nodes), k + 1), -1.0)
    if case.offspring:
        for n, gl in enumerate(ns["compute_gt_likelihoods"](case.progeny_table, case.offspring[0], pairs, info, case.param)):
            if gl:
                plain[n] = gl
    rec["f64_no_priors_sample0"] = gc.pack(plain, "<f8")
    # against the exact rationals; the reference's normalising sums
    prev = None
    margins = []
    for n, (v, pos) in enumerate(pairs):
        if pos == prev:
            continue
        prev = pos
        var = info[v]
        for s, sample in enumerate(case.offspring):
            d = case.progeny_table.allele_depths_of(sample)[pos]
            ref_dp = d[var.ref] if len(d) > var.ref else 0
            alt_dp = d[var.alt] if len(d) > var.alt else 0
            if ref_dp + alt_dp < k:
                assert f64[n, s, 0] == -1.0
                continue
            for prior, got in ((priors[var.alt_count][var.co_alt_count], f64[n, s]), (None, plain[n] if s == 0 else None)):
                if got is None:
                    continue
                pmf = [ns["get_binom_pmf"](ref_dp + alt_dp, alt_dp, g, k, case.param.allele_error_rate) * (prior[g] if prior else 1.0) for g in range(k + 1)]
                totals["min_sum"] = min(totals["min_sum"], sum(pmf))
                for g, exact in enumerate(gc.exact_cell(ref_dp, alt_dp, k, case.param.allele_error_rate, prior)):
                    if exact == 0:
                        assert got[g] == 0.0
                        continue
                    totals["e_ref"] = max(totals["e_ref"], float(abs(Fraction(float(got[g])) - exact) / exact))
                    if prior:
                        margins.append((boundary_distance(float(got[g])), spec["name"], n, s, g))
    # correct_variant_types on a fresh VariantInfo
    info = case.varinfo(ns["VariantInfo"])
    ns["correct_variant_types"](case.variant_table, case.progeny_table, case.offspring, info, case.param)
    rec["after_correct"] = gc.state_of(info)
    return rec, margins


def record_underflowing(ns):
    """What the reference does with the cells of progeny_gl_cases.UNDERFLOWING (ploidy 4, error rate 0.06, no priors): its normalising sum
    and whether compute_gt_likelihoods raises ZeroDivisionError or returns NaN."""
    out = []
    for ref_dp, alt_dp in gc.UNDERFLOWING:
        pmf = [ns["get_binom_pmf"](ref_dp + alt_dp, alt_dp, g, 4, 0.06) for g in range(5)]
        info = ns["VariantInfo"]([gc.SN])
        info.append(0, 1, 1, 0)
        try:
            with np.errstate(all="ignore"):
                gl = ns["compute_gt_likelihoods"](gc.Table([100], {"s": [(ref_dp, alt_dp)]}), "s", [(0, 0)], info, gc.Param(4, 0.06))[0]
            outcome = "nan" if all(math.isnan(x) for x in gl) else "values"
        except ZeroDivisionError:
            outcome = "ZeroDivisionError"
        out.append(dict(ref_dp=ref_dp, alt_dp=alt_dp, ploidy=4, error_rate=0.06, normalising_sum=float(sum(pmf)).hex(), outcome=outcome))
    return out


def baseline(ref_root, n_nodes):
    """The reference's get_offspring_gl on the compiled class: the first n_nodes nodes of progeny_gl_cases.large_depth_problem()."""
    import time

    with tempfile.TemporaryDirectory() as tmp:
        L = base.build_wrapper(ref_root, tmp)
        ns = load_reference(ref_root, L)
        tables = gc.large_tables(n_nodes)
        info = tables.varinfo(ns["VariantInfo"])
        t0 = time.perf_counter()
        off_gl = ns["get_offspring_gl"](tables.variant_table, tables.progeny_table, tables.offspring, info, tables.param)
        t1 = time.perf_counter()
        n, s = off_gl.getNumPositions(), off_gl.getNumSamples()
        off_gl.close()
    print(json.dumps({"nodes": n, "samples": s, "ploidy": tables.param.ploidy, "cells": n * s, "get_offspring_gl_s": round(t1 - t0, 3),
                      "cells_per_s": n * s / (t1 - t0)}))


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("WHATSHAP_REFERENCE", "")
    if not ref_root or not os.path.isdir(os.path.join(ref_root, "src", "polyphase")):
        sys.exit("usage: make_progeny_gl_golden.py /path/to/reference (a WhatsHap source tree)")
    if len(sys.argv) > 3 and sys.argv[2] == "--baseline":
        return baseline(ref_root, int(sys.argv[3]))
    totals = {"e_ref": 0.0, "min_sum": math.inf}
    cases, margins = [], []
    with tempfile.TemporaryDirectory() as tmp:
        L = base.build_wrapper(ref_root, tmp)
        ns = load_reference(ref_root, L)
        for spec in gc.specs():
            assert spec["max_depth"] <= 120 and spec["ploidy"] <= 8   # (deeper or wider: check the normalising sums again)
            rec, m = record_case(ns, spec, totals)
            cases.append(rec)
            margins += m
        underflowing = record_underflowing(ns)
    assert totals["min_sum"] > 1e-280, f"a normalising sum of the reference fell to {totals['min_sum']}"
    close = [m for m in margins if m[0] <= 10 * totals["e_ref"]]
    assert not close, f"doubles within 10 * E_ref = {10 * totals['e_ref']} of a float rounding boundary (distance, case, node, sample, genotype): {close}"
    with gzip.GzipFile(OUT, "wb", mtime=0) as f:
        f.write(json.dumps({"cases": cases, "e_ref": totals["e_ref"].hex(), "min_sum": totals["min_sum"].hex(), "underflowing": underflowing}, separators=(",", ":")).encode())
    print(f"{len(cases)} cases, {sum(len(c['nodes']) * c['spec']['n_samples'] for c in cases)} cells, E_ref {totals['e_ref']:.3g}, smallest normalising sum "
          f"{totals['min_sum']:.3g}, smallest boundary distance {min(m[0] for m in margins):.3g} -> {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
