#!/usr/bin/env python3
"""Writes tests/golden/readmerge_cases.json.gz: what the reference's ReadMerger.merge returns for the cases of tests/readmerge_cases.py
(run only where the reference tree exists; the tests read the recorded data).

whatshap/merge.py imports the compiled core, which need not be installed: at generation time the file is parsed, its imports are
dropped and the rest is executed with stand-ins for what it uses (``Read`` / ``ReadSet``: this package's classes; ``nx``: a thin proxy
over the real networkx whose ``Graph`` records every ``add_edge``, so that the blue and the not-blue edges and their match / mismatch
are captured as well; ``logger``: silent).  Nothing of the reference is written out.

Recorded per case: the spec (tests/readmerge_cases.py generates the input from it), the SHA-256 of the generated input, the blue and
the not-blue edges in the order the reference added them, the representatives read off its blue graph after the edge removal, and
the merged reads -- or the exception class.
Usage: python tests/golden/make_readmerge_golden.py /path/to/reference
       python tests/golden/make_readmerge_golden.py /path/to/reference --baseline 2000
           (writes nothing: times the reference's own merge on the first 2 000 reads of the benchmark's read set, one thread -- the
           figure of profiles/readmerge/cpu_baseline.md)
"""
import abc
import ast
import gzip
import json
import math
import os
import sys
import typing

import networkx

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "readmerge_cases.json.gz")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import readmerge_cases as rc  # noqa: E402
from whatshap_amd.core import Read, ReadSet  # noqa: E402


class _Logger:
    def debug(self, *a, **k):
        pass

    info = warning = error = debug


class _NxProxy:
    """networkx, except that every Graph made through it is kept and records its add_edge calls."""

    def __init__(self):
        self.graphs = []
        proxy = self

        class Graph(networkx.Graph):
            def __init__(self, *a, **k):
                super().__init__(*a, **k)
                self.added = []
                proxy.graphs.append(self)

            def add_edge(self, u, v, **attr):
                self.added.append([int(u), int(v), int(attr["match"]), int(attr["mismatch"])])
                super().add_edge(u, v, **attr)

        self.Graph = Graph

    def __getattr__(self, name):
        return getattr(networkx, name)


def load_reference(ref_root):
    """The reference's merge.py without its imports, compiled from its own text at run time."""
    path = os.path.join(ref_root, "whatshap", "merge.py")
    tree = ast.parse(open(path).read(), filename=path)
    keep = [n for n in tree.body if not isinstance(n, (ast.Import, ast.ImportFrom))]
    ns = {"nx": _NxProxy(), "log": math.log, "Read": Read, "ReadSet": ReadSet, "logging": None, "ABC": abc.ABC, "abstractmethod": abc.abstractmethod,
          "Dict": typing.Dict, "__name__": "reference_merge"}
    keep = [n for n in keep if not (isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "logger")]
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    ns["logger"] = _Logger()
    return ns


def record(ns, spec):
    data = rc.materialize(spec)
    rec = dict(spec={k: v for k, v in spec.items() if k != "data"} if spec["kind"] == "explicit" else spec, input_sha256=rc.input_sha256(data), raises=None)
    proxy = ns["nx"]
    del proxy.graphs[:]
    try:
        merged = ns["ReadMerger"](*rc.merger_args(spec)).merge(rc.readset_of(data))
    except Exception as e:
        rec["raises"] = type(e).__name__
        return rec
    blue, not_blue = proxy.graphs   # in the order merge() makes them
    representative = list(range(len(data["reads"])))
    for members in networkx.connected_components(blue):
        for v in members:
            representative[v] = min(members)
    rec["results"] = dict(blue=blue.added, not_blue=not_blue.added, representative=representative, merged=rc.canonical_reads(merged))
    return rec


def baseline(ref_root, n_reads):
    import time

    ns = load_reference(ref_root)
    read_ptr, position, allele, quality = rc.bench_reads(n_reads=n_reads)
    rs = ReadSet()
    for r in range(read_ptr.size - 1):
        read = Read(f"r{r}")
        for x in range(int(read_ptr[r]), int(read_ptr[r + 1])):
            read.add_variant(int(position[x]), int(allele[x]), int(quality[x]))
        rs.add(read)
    t0 = time.perf_counter()
    merged = ns["ReadMerger"](0.15, 0.25, 1000000, 1000).merge(rs)
    t1 = time.perf_counter()
    blue = ns["nx"].graphs[0]
    print(json.dumps({"reads": len(rs), "entries": int(read_ptr[-1]), "blue_edges": len(blue.added), "merged_reads": len(merged), "merge_s": round(t1 - t0, 3),
                      "reads_per_s": len(rs) / (t1 - t0)}))


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("WHATSHAP_REFERENCE", "")
    if not ref_root or not os.path.isfile(os.path.join(ref_root, "whatshap", "merge.py")):
        sys.exit("usage: make_readmerge_golden.py /path/to/reference (a WhatsHap source tree)")
    if len(sys.argv) > 3 and sys.argv[2] == "--baseline":
        return baseline(ref_root, int(sys.argv[3]))
    ns = load_reference(ref_root)
    cases = [record(ns, spec) for spec in rc.all_specs()]
    with gzip.GzipFile(OUT, "wb", mtime=0) as f:
        f.write(json.dumps({"cases": cases}, separators=(",", ":")).encode())
    done = [c for c in cases if not c["raises"]]
    print(f"{len(cases)} cases ({len(cases) - len(done)} raise, {sum(len(c['results']['blue']) for c in done)} blue edges, "
          f"{sum(1 for c in done if c['results']['not_blue'])} with not-blue edges) -> {OUT} ({os.path.getsize(OUT)} bytes)")
    for c in done:
        r = c["results"]
        n = len(r["representative"])
        uncut = list(range(n))   # the components of ALL blue edges: differs from the recorded ones where the removal loop cut
        for j, i, _, _ in sorted(r["blue"]):
            a, b = uncut[j], uncut[i]
            if a != b:
                uncut = [min(a, b) if x in (a, b) else x for x in uncut]
        print(" ", c["spec"]["name"], "reads", n, "blue", len(r["blue"]), "not blue", len(r["not_blue"]), "merged", len(r["merged"]),
              "CUT" if uncut != r["representative"] else "")
    for c in cases:
        if c["raises"]:
            print(" ", c["spec"]["name"], c["raises"])


if __name__ == "__main__":
    main()
