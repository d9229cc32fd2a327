#!/usr/bin/env python3
"""Writes tests/golden/prior_genotype_cases.json.gz: what the reference's compute_genotypes (core.pyx:603 over src/genotyper.cpp, from
the extension modules of oracle/_ref/cy) and the regularisation loop of its cli/genotype.py return for the cases of
tests/prior_genotype_cases.py.  Run only where the reference tree exists; the tests read the recorded data.

whatshap/cli/genotype.py imports pysam and the rest of the command line, which need not be installed: at generation time the file is
parsed and only ``int_to_diploid_biallelic_gt``, ``determine_genotype`` and the loop of ``run_genotype`` over ``genotype_likelihoods``
are executed, on the reference's own ``Genotype`` and ``PhredGenotypeLikelihoods``.  Nothing of the reference is written out.

Recorded per case: its input arrays, the likelihoods as float.hex(), the genotypes (0 .. 2, -1: none) and -- where the case carries a
constant and a threshold -- the regularised likelihoods and genotypes.

Two conditions are asserted before anything is written:
  1. at least half of the columns with two or more counted entries change bits when their entries are reversed (plain-Python chain): the
     fixture can tell an ordered run from an unordered one;
  2. every column's plain-Python chain equals the reference exactly: the fixture itself is sound.

Usage: python tests/golden/make_prior_genotype_golden.py /path/to/reference
       python tests/golden/make_prior_genotype_golden.py /path/to/reference --baseline 20000
           (writes nothing: times the reference's compute_genotypes and the Python loop on the first 20 000 positions' worth of the
           benchmark's problem, one thread -- the figure of profiles/prior_genotypes/cpu_baseline.md)
"""
import ast
import gzip
import json
import os
import sys
import typing

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "prior_genotype_cases.json.gz")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import prior_genotype_cases as pc  # noqa: E402
from oracle import build_cython_ref  # noqa: E402


def load_reference_tail(ref_root, ref):
    """determine_genotype and the regularisation loop, compiled from the reference's own text at run time: a function
    tail(genotype_likelihoods, genotypes, constant, gt_prob) -> (genotypes, reg_genotype_likelihoods)."""
    path = os.path.join(ref_root, "whatshap", "cli", "genotype.py")
    tree = ast.parse(open(path).read(), filename=path)
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("int_to_diploid_biallelic_gt", "determine_genotype")]
    assert len(keep) == 2
    run = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "run_genotype")
    loops = [n for n in ast.walk(run) if isinstance(n, ast.For) and isinstance(n.target, ast.Name) and n.target.id == "gl"]
    assert len(loops) == 1, "the regularisation loop of run_genotype was not found"
    ns = {"Genotype": ref.Genotype, "PhredGenotypeLikelihoods": ref.PhredGenotypeLikelihoods}
    ns.update({k: getattr(typing, k) for k in ("List", "Optional", "Sequence", "Dict", "Tuple")})
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    loop = compile(ast.Module(body=loops, type_ignores=[]), path, "exec")

    def tail(genotype_likelihoods, genotypes, constant, gt_prob):
        scope = dict(ns, genotype_likelihoods=genotype_likelihoods, genotypes=list(genotypes), constant=constant, gt_prob=gt_prob, reg_genotype_likelihoods=[])
        exec(loop, scope)
        return scope["genotypes"], scope["reg_genotype_likelihoods"]

    return tail


def genotype_code(g):
    alleles = list(g.as_vector())
    return sum(alleles) if len(alleles) == 2 else -1


def record(ref, tail, case):
    readset = pc.readset_of(case, ref)
    genotypes, gls = ref.compute_genotypes(readset, case["positions"])
    rec = dict(case, gl=[pc.hex3(g) for g in gls], gt=[genotype_code(g) for g in genotypes])
    if case["constant"] is not None:
        reg_genotypes, reg = tail(gls, genotypes, case["constant"], pc.gt_prob_of(case))
        rec["reg"] = [pc.hex3(list(r)) for r in reg]
        rec["reg_gt"] = [genotype_code(g) for g in reg_genotypes]
    return rec


def check_fixture(records):
    deep = changed = 0
    for rec in records:
        columns = pc.columns_of(rec)
        assert len(columns) == len(rec["gl"]), rec["name"]
        for entries, want, gt in zip(columns, rec["gl"], rec["gt"]):
            got = pc.python_chain(entries)
            assert pc.hex3(got) == want, (rec["name"], entries[:8], pc.hex3(got), want)   # condition 2
            assert pc.python_genotype(got) == gt, rec["name"]
            if len(entries) >= 2:
                deep += 1
                changed += pc.hex3(pc.python_chain(entries[::-1])) != want
    assert deep and 2 * changed >= deep, f"only {changed} of {deep} columns depend on the order of their entries"   # condition 1
    return deep, changed


def baseline(ref_root, ref, n_positions):
    import time

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "scripts"))
    import gpu_prior_genotypes_bench as bench

    case = bench.bench_arrays(n_positions=n_positions, n_reads=2 * n_positions)
    tail = load_reference_tail(ref_root, ref)
    readset = ref.ReadSet()
    ptr, pos, allele, qual = case
    for r in range(len(ptr) - 1):
        read = ref.Read(f"r{r}", 60, 0, 0)
        for x in range(int(ptr[r]), int(ptr[r + 1])):
            read.add_variant(int(pos[x]), int(allele[x]), int(qual[x]))
        readset.add(read)
    positions = list(range(n_positions))
    t0 = time.perf_counter()
    genotypes, gls = ref.compute_genotypes(readset, positions)
    t1 = time.perf_counter()
    tail(gls, genotypes, 0.0, 0.0)
    t2 = time.perf_counter()
    print(json.dumps({"positions": n_positions, "reads": len(ptr) - 1, "entries": int(ptr[-1]), "compute_genotypes_s": round(t1 - t0, 3),
                      "python_loop_s": round(t2 - t1, 3), "positions_per_s": n_positions / (t2 - t0)}))


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("WHATSHAP_REFERENCE", "")
    if not ref_root or not os.path.isfile(os.path.join(ref_root, "whatshap", "cli", "genotype.py")):
        sys.exit("usage: make_prior_genotype_golden.py /path/to/reference (a WhatsHap source tree)")
    ref = build_cython_ref.import_reference()
    if len(sys.argv) > 3 and sys.argv[2] == "--baseline":
        return baseline(ref_root, ref, int(sys.argv[3]))
    tail = load_reference_tail(ref_root, ref)
    records = [record(ref, tail, case) for case in pc.all_cases()]
    deep, changed = check_fixture(records)
    with gzip.GzipFile(OUT, "wb", mtime=0) as f:
        f.write(json.dumps({"cases": records}, separators=(",", ":")).encode())
    print(f"{len(records)} cases, {sum(len(r['gl']) for r in records)} columns; {changed} of {deep} columns with two or more counted entries change bits "
          f"when reversed -> {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
