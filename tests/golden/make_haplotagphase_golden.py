#!/usr/bin/env python3
"""Writes tests/golden/haplotagphase_cases.json.gz: what the reference's compute_votes and consensus return for the cases of
tests/haplotagphase_cases.py (run only where the reference tree exists; the tests read the recorded data).

whatshap/cli/haplotagphase.py imports pysam, pyfaidx and the compiled core, which need not be installed: at generation time the file is
parsed and only ``compute_votes``, ``consensus``, ``best_candidate`` and ``length_of_homopolymer`` are executed, with stand-ins for what
they use (``logger``: keeps the warnings, from which the number of skipped reads is read; ``Variant``: this package's dataclass; reads and
variants: the stand-ins of tests/haplotagphase_cases.py).  Nothing of the reference is written out.

Recorded per case: the spec (tests/haplotagphase_cases.py generates the input from it), the SHA-256 of the generated input, the votes dict
in its own order, the number of skipped reads, the two superreads and the components in their order -- or, from the function that raises
on, the exception class.
Usage: python tests/golden/make_haplotagphase_golden.py /path/to/reference
       python tests/golden/make_haplotagphase_golden.py /path/to/reference --baseline 20000
           (writes nothing: times the reference's own two functions on the first 20 000 reads of the benchmark's problem, one thread -- the
           figure of profiles/haplotagphase/cpu_baseline.md)
"""
import ast
import gzip
import itertools
import json
import os
import sys
import typing

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "haplotagphase_cases.json.gz")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import haplotagphase_cases as hc  # noqa: E402
from whatshap_amd.core import Read, Variant  # noqa: E402

WANTED = ("compute_votes", "consensus", "best_candidate", "length_of_homopolymer")


class _Logger:
    def __init__(self):
        self.warnings = []

    def warning(self, msg, *a, **k):
        self.warnings.append(str(msg))

    def debug(self, *a, **k):
        pass

    info = error = debug


def load_reference_functions(ref_root):
    """The wanted definitions of the reference's haplotagphase.py, compiled from its own text at run time."""
    path = os.path.join(ref_root, "whatshap", "cli", "haplotagphase.py")
    tree = ast.parse(open(path).read(), filename=path)
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in WANTED]
    assert sorted(n.name for n in keep) == sorted(WANTED)
    ns = {"itertools": itertools, "logger": _Logger(), "Variant": Variant, "Read": object, "VcfVariant": object, "VariantCallPhase": object}
    ns.update({k: getattr(typing, k) for k in ("List", "Optional", "Union", "Dict", "Tuple", "Sequence")})
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns


def skipped_of(logger):
    """The count the reference's warning starts with (no warning: none skipped)."""
    assert len(logger.warnings) <= 1
    return int(logger.warnings[0].split()[0]) if logger.warnings else 0


def record(ns, spec):
    data = hc.materialize(spec)
    rec = dict(spec={k: v for k, v in spec.items() if k != "data"} if spec["kind"] == "explicit" else spec, input_sha256=hc.input_sha256(data), raises=None)
    args = hc.call_args(data)
    ns["logger"].warnings.clear()
    try:
        votes = ns["compute_votes"](args["is_homozygous"], args["reads"], args["allele_to_id"])
    except Exception as e:
        rec["raises"] = type(e).__name__
        rec["raised_by"] = "compute_votes"
        return rec
    skipped = skipped_of(ns["logger"])
    try:
        super_reads, components = ns["consensus"](spec["only_indels"], spec["gap_threshold"], spec["cut_homopolymers"], args["refseq"], args["change"],
                                                  args["phased"], votes, args["id_to_allele"])
    except Exception as e:
        rec["raises"] = type(e).__name__
        rec["raised_by"] = "consensus"
        rec["results"] = hc.canonical(votes, [[], []], {}, skipped)
        return rec
    rec["results"] = hc.canonical(votes, super_reads, components, skipped)
    return rec


def baseline(ref_root, n_reads):
    """The reference's own two functions on the first n_reads reads of haplotagphase_cases.bench_problem(), through stand-in objects that
    hold the same arrays."""
    import time

    ns = load_reference_functions(ref_root)
    p = hc.bench_problem(n_reads=n_reads)
    n_var = p.variant_flags.size
    hom = {x: bool(p.variant_flags[x] & 1) for x in range(n_var)}
    phased = {x: (object() if p.variant_flags[x] & 2 else None) for x in range(n_var)}
    snv, indel = hc._Change(True), hc._Change(False)
    change = {x: (snv if p.variant_flags[x] & 4 else indel) for x in range(n_var)}
    ids = {x: {0: 0, 1: 1} for x in range(n_var)}
    reads = []
    for r in range(p.n_reads):
        read = Read(f"r{r}", 0, 0, 0, 0, "", int(p.read_hp[r]) + 1, int(p.read_ps[r]) + 1)
        for x in range(int(p.read_ptr[r]), int(p.read_ptr[r + 1])):
            read.add_variant(int(p.entry_variant[x]), int(p.entry_id[x]), int(p.entry_quality[x]))
        reads.append(read)
    t0 = time.perf_counter()
    votes = ns["compute_votes"](hom, reads, ids)
    t1 = time.perf_counter()
    super_reads, components = ns["consensus"](p.only_indels, p.gap_threshold, 0, "", change, phased, votes, ids)
    t2 = time.perf_counter()
    n_entries = int(p.read_ptr[-1])
    print(json.dumps({"reads": p.n_reads, "entries": n_entries, "variants": n_var, "voted": len(votes), "kept": len(super_reads[0]),
                      "skipped": skipped_of(ns["logger"]), "compute_votes_s": round(t1 - t0, 3), "consensus_s": round(t2 - t1, 3),
                      "entries_per_s": n_entries / (t2 - t0), "reads_per_s": p.n_reads / (t2 - t0)}))


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("WHATSHAP_REFERENCE", "")
    if not ref_root or not os.path.isfile(os.path.join(ref_root, "whatshap", "cli", "haplotagphase.py")):
        sys.exit("usage: make_haplotagphase_golden.py /path/to/reference (a WhatsHap source tree)")
    if len(sys.argv) > 3 and sys.argv[2] == "--baseline":
        return baseline(ref_root, int(sys.argv[3]))
    ns = load_reference_functions(ref_root)
    cases = [record(ns, spec) for spec in hc.all_specs()]
    with gzip.GzipFile(OUT, "wb", mtime=0) as f:
        f.write(json.dumps({"cases": cases}, separators=(",", ":")).encode())
    print(f"{len(cases)} cases ({sum(1 for c in cases if c['raises'])} raise, {sum(len(c['results']['votes']) for c in cases if 'results' in c)} voted positions, "
          f"{sum(len(c['results']['super_reads'][0]) for c in cases if 'results' in c)} kept) -> {OUT} ({os.path.getsize(OUT)} bytes)")
    for c in cases:
        print(" ", c["spec"]["name"], c["raises"] or (len(c["results"]["votes"]), len(c["results"]["super_reads"][0]), c["results"]["skipped"]))


if __name__ == "__main__":
    main()
