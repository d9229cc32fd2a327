#!/usr/bin/env python3
"""Writes tests/golden/haplotag_cases.json.gz: what the reference's prepare_haplotag_information returns for the cases of
tests/haplotag_cases.py (run only where the reference tree exists; the tests read the recorded data).

whatshap/cli/haplotag.py imports pysam and xopen, which need not be installed: at generation time the file is parsed and only
``SupplementaryHaplotaggingStrategy``, ``get_variant_information``, the two dataclasses, ``read_representation`` and
``prepare_haplotag_information`` are executed, with stand-ins for what they import (``logger``: silent; ``PRIMARY_DEFAULT_SUB_ALIGNMENT_ID``:
the literal of whatshap/variants.py, read from its text).  Nothing of the reference is written out.

Recorded per case: the spec (tests/haplotag_cases.py generates the input from it), the SHA-256 of the generated input, and the reference's
complete results -- every assigned representation with (haplotype, quality, phase set), the BX lists in order, n_multiple_phase_sets,
primary_info_by_repr -- or the exception class where it raises.

The reference iterates a group of several linked reads as a ``set``, so the order in which such a group first meets its phase sets is
arbitrary; it decides only a tie between two phase sets on the largest haplotype sum.  The running function is watched at the statement
after its sort: the generator FAILS -- it drops nothing -- if a group of more than one read has two phase sets sharing the top maximum.
Usage: python tests/golden/make_haplotag_golden.py /path/to/reference
       python tests/golden/make_haplotag_golden.py /path/to/reference --baseline 20000
           (writes nothing: times the reference's own loop on the first 20 000 reads of the benchmark's long-read problem, one thread --
           the figure of profiles/haplotag/cpu_baseline.md)
"""
import ast
import dataclasses
import enum
import gzip
import json
import os
import sys
import typing
from collections import defaultdict

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "haplotag_cases.json.gz")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import haplotag_cases as hc  # noqa: E402

WANTED = ("SupplementaryHaplotaggingStrategy", "get_variant_information", "ReadAlignmentRepresentation", "PrimaryInfo", "read_representation",
          "prepare_haplotag_information")


class _SilentLogger:
    def debug(self, *a, **k):
        pass

    info = warning = error = debug


def load_reference_functions(ref_root):
    """The wanted definitions of the reference's haplotag.py, compiled from its own text at run time, and
    the line of prepare_haplotag_information's ``if len(l) == 0`` -- the statement after its sort."""
    variants_py = os.path.join(ref_root, "whatshap", "variants.py")
    default_id = None
    for node in ast.parse(open(variants_py).read()).body:
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", "") == "PRIMARY_DEFAULT_SUB_ALIGNMENT_ID":
            default_id = ast.literal_eval(node.value)
    assert isinstance(default_id, str)
    path = os.path.join(ref_root, "whatshap", "cli", "haplotag.py")
    tree = ast.parse(open(path).read(), filename=path)
    keep = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in WANTED]
    assert sorted(n.name for n in keep) == sorted(WANTED)
    ns = {"dataclass": dataclasses.dataclass, "Enum": enum.Enum, "defaultdict": defaultdict, "logger": _SilentLogger(),
          "PRIMARY_DEFAULT_SUB_ALIGNMENT_ID": default_id, "VariantTable": object, "VariantCallPhase": object, "Read": object}   # (the last three: annotations)
    ns.update({k: getattr(typing, k) for k in ("List", "Optional", "Union", "Dict", "Tuple", "FrozenSet", "Sequence", "TextIO")})
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    fn = next(n for n in keep if n.name == "prepare_haplotag_information")
    after_sort = [n for n in ast.walk(fn) if isinstance(n, ast.If) and isinstance(n.test, ast.Compare) and isinstance(n.test.left, ast.Call)
                  and getattr(n.test.left.func, "id", "") == "len" and getattr(n.test.left.args[0], "id", "") == "l"
                  and isinstance(n.test.ops[0], ast.Eq) and getattr(n.test.comparators[0], "value", None) == 0]
    assert len(after_sort) == 1
    return ns, after_sort[0].lineno


def run_watched(ns, line, args, name):
    """prepare_haplotag_information(*args) with the multi-read tie check; returns (results, groups seen, multi-read groups seen)."""
    seen = [0, 0]

    def tracer(frame, event, arg):
        if frame.f_code.co_name != "prepare_haplotag_information":
            return None
        if event == "line" and frame.f_lineno == line:
            costs, group = frame.f_locals["l"], frame.f_locals["reads_to_consider"]
            seen[0] += 1
            if len(group) > 1:
                seen[1] += 1
                if len(costs) > 1 and max(costs[0][1]) == max(costs[1][1]):
                    raise SystemExit(f"case {name}: a group of {len(group)} reads has two phase sets sharing the top maximum {max(costs[0][1])}: "
                                     "the reference's result depends on its set order -- choose another seed")
        return tracer

    sys.settrace(tracer)
    try:
        results = ns["prepare_haplotag_information"](*args)
    finally:
        sys.settrace(None)
    return results, seen[0], seen[1]


def record(ns, line, spec):
    data = hc.materialize(spec)
    rec = dict(spec={k: v for k, v in spec.items() if k != "data"} if spec["kind"] == "explicit" else spec, input_sha256=hc.input_sha256(data))
    try:
        results, n_groups, n_multi = run_watched(ns, line, hc.call_args(spec, data), spec["name"])
    except Exception as e:   # (SystemExit of the tie check is not an Exception: it ends the run)
        rec["raises"] = type(e).__name__
        return rec
    rec["raises"] = None
    rec["groups_with_variants_or_not"] = n_groups
    rec["multi_read_groups"] = n_multi
    rec["results"] = hc.canonical(results)
    return rec


def baseline(ref_root, n_reads):
    """The reference's own loop on the first n_reads reads of haplotag_cases.bench_problem("long2"), through stand-in objects that hold the
    same arrays."""
    import time

    ns, _ = load_reference_functions(ref_root)
    p = hc.bench_problem("long2", n_reads=n_reads)
    phasing = [tuple(int(a) for a in row) for row in p.variant_phasing]
    info = {int(pos): (int(ps), ph) for pos, ps, ph in zip(p.variant_position, p.variant_phaseset, phasing)}
    ns["get_variant_information"] = lambda table, sample: (info, [])
    reads = []
    for r in range(p.n_reads):
        read = hc.Read(f"r{r}____1", 0, 0, 0, int(p.read_start[r]), "", -1, -1, hc.CHROMOSOME, "____1", False, int(p.read_start[r]) + 1, False)
        for x in range(int(p.read_ptr[r]), int(p.read_ptr[r + 1])):
            read.add_variant(int(p.entry_position[x]), int(p.entry_allele[x]), int(p.entry_quality[x]))
        reads.append(read)

    class Reader:
        def read(self, *a, **k):
            return reads, None

    class Table:
        chromosome = hc.CHROMOSOME

    t0 = time.perf_counter()
    _, assigned, n_multiple, _ = ns["prepare_haplotag_information"](Table(), ["s0"], Reader(), None, True, 50000, 2)
    t1 = time.perf_counter()
    n_entries = int(p.read_ptr[-1])
    print(json.dumps({"reads": p.n_reads, "entries": n_entries, "assigned": len(assigned), "n_multiple_phase_sets": n_multiple,
                      "prepare_haplotag_information_s": round(t1 - t0, 3), "entries_per_s": n_entries / (t1 - t0), "reads_per_s": p.n_reads / (t1 - t0)}))


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("WHATSHAP_REFERENCE", "")
    if not ref_root or not os.path.isfile(os.path.join(ref_root, "whatshap", "cli", "haplotag.py")):
        sys.exit("usage: make_haplotag_golden.py /path/to/reference (a WhatsHap source tree)")
    if len(sys.argv) > 3 and sys.argv[2] == "--baseline":
        return baseline(ref_root, int(sys.argv[3]))
    ns, line = load_reference_functions(ref_root)
    cases = [record(ns, line, spec) for spec in hc.all_specs()]
    with gzip.GzipFile(OUT, "wb", mtime=0) as f:
        f.write(json.dumps({"cases": cases}, separators=(",", ":")).encode())
    print(f"{len(cases)} cases ({sum(1 for c in cases if c['raises'])} raise, {sum(c.get('multi_read_groups', 0) for c in cases)} multi-read groups, "
          f"{sum(len(c['results']['reads']) for c in cases if not c['raises'])} assigned representations) -> {OUT} ({os.path.getsize(OUT)} bytes)")
    for c in cases:
        print(" ", c["spec"]["name"], c["raises"] or (len(c["results"]["reads"]), c["results"]["n_multiple_phase_sets"], len(c["results"]["bx"])))


if __name__ == "__main__":
    main()
