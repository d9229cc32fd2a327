#!/usr/bin/env python3
"""Writes tests/golden/realign_cases.json.gz: what the reference's allele detection by re-alignment returns (run only where the
reference tree exists; the tests read the recorded data).

The reference's whatshap/align.pyx and whatshap/_variants.pyx are compiled with Cython in C++ mode (as its setup.py builds them) into a
temporary directory outside the repository, and its whatshap/variants.py is imported there with stand-ins for pysam, pyfaidx-free
whatshap.vcf / whatshap.bam and whatshap.core (none of which ReadSetReader.realign uses).  Recorded:
  (a) "pairs":  edit_distance / edit_distance_affine_gap of >= 2000 pairs (lengths 0 - 200, shared prefixes and suffixes, mismatch costs
                with 15.1 and 0.3, gaps (1, 1), (10, 7), (10.5, 7));
  (b) "groups": detect_alleles_by_alignment over synthetic references, variants (SNV, indels up to 30 bp, MNV, multi-allelic, symbolic,
                two at one position) and alignments with every CIGAR operation, overhang 3 / 10 / 25, both cost models, restricted
                genotypes; every read's yields, or the exception the reference raised for it ("errors").
and, to tests/golden/realign_edge_cases.json.gz:
  (c) edit_distance / edit_distance_affine_gap of every pair of tests/realign_cases.py edge_pairs() (query words 63 | 64 | 65 and
      127 | 128 | 129, the same for the target's carry words, targets at 1364 | 1365 and 5460 | 5461, gaps beyond 2^24): the results
      in the generator's order and a hash of the generated inputs, no sequences.
Usage: python tests/golden/make_realign_golden.py [--edge-only] [/path/to/reference]     (--edge-only: (c) alone)
"""
import gzip
import importlib.util
import json
import os
import random
import shutil
import subprocess
import sys
import sysconfig
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "realign_cases.json.gz")
OUT_EDGE = os.path.join(HERE, "realign_edge_cases.json.gz")


def build_reference(ref_root, tmp):
    pkg = os.path.join(tmp, "whatshap")
    os.makedirs(pkg)
    inc = sysconfig.get_paths()["include"]
    suffix = sysconfig.get_config_var("EXT_SUFFIX")
    for mod in ("align", "_variants"):
        cpp = os.path.join(tmp, mod + ".cpp")
        subprocess.run([sys.executable, "-m", "cython", "--cplus", "-3", os.path.join(ref_root, "whatshap", mod + ".pyx"), "-o", cpp], check=True)
        subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-I" + inc, cpp, "-o", os.path.join(pkg, mod + suffix)], check=True)
    open(os.path.join(pkg, "__init__.py"), "w").close()
    sys.path.insert(0, tmp)
    # stand-ins for what variants.py imports and realign does not use
    pysam = types.ModuleType("pysam")
    pysam.AlignedSegment = object
    sys.modules["pysam"] = pysam
    for name, attrs in (("whatshap.vcf", ("VcfVariant",)), ("whatshap.bam", ("SampleBamReader", "MultiBamReader", "BamReader", "AlignmentWithSourceID")),
                        ("whatshap.core", ("Genotype", "Read", "ReadSet", "NumericSampleIds"))):
        m = types.ModuleType(name)
        for a in attrs:
            setattr(m, a, type(a, (), {}))
        sys.modules[name] = m
    import whatshap  # noqa: F401
    spec = importlib.util.spec_from_file_location("whatshap.variants", os.path.join(ref_root, "whatshap", "variants.py"))
    variants = importlib.util.module_from_spec(spec)
    sys.modules["whatshap.variants"] = variants
    spec.loader.exec_module(variants)
    from whatshap import align

    return align, variants


class Var:
    def __init__(self, position, ref, alts):
        self.position, self.reference_allele, self._alts = position, ref, list(alts)

    def get_alt_allele_list(self):
        return self._alts


class Gt:
    def __init__(self, alleles):
        self._a = list(alleles)

    def as_vector(self):
        return self._a


class Aln:
    def __init__(self, start, cigar, seq):
        self.reference_start, self.cigartuples, self.query_sequence = start, cigar, seq


def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def make_pairs(rng, align):
    out = []
    for k in range(2400):
        kind = k % 4
        n = rng.choice([0, 1, 2, 5, 10, 21, 40, 63, 64, 65, 100, 127, 128, 129, 200]) if rng.random() < 0.5 else rng.randint(0, 200)
        alphabet = "ACGT" if rng.random() < 0.8 else "ACGTNacgt"
        s = rand_seq(rng, n, alphabet)
        t = list(s)
        for _ in range(rng.randint(0, max(1, n // 5))):   # edits keep long shared prefixes / suffixes
            op, p = rng.random(), rng.randint(0, len(t))
            if op < 0.4 and p < len(t):
                t[p] = rng.choice("ACGTN")
            elif op < 0.7:
                t[p:p] = list(rand_seq(rng, rng.randint(1, 12)))
            elif p < len(t):
                del t[p:p + rng.randint(1, 12)]
        t = "".join(t) if rng.random() < 0.9 else rand_seq(rng, rng.randint(0, 200))
        t = t[:200]
        if kind < 2:
            out.append({"q": s, "t": t, "unit": align.edit_distance(s, t)})
        gs, ge = rng.choice([(1, 1), (10, 7), (10.5, 7)])
        if rng.random() < 0.5:
            costs = [rng.choice([15.1, 0.3, 1.0, 7.7]) for _ in s]
        else:
            costs = [rng.choice([15.1, 0.3])] * len(s)
        out.append({"q": s, "t": t, "costs": costs, "gap": [gs, ge], "affine": align.edit_distance_affine_gap(s, t, costs, gs, ge)})
    return out


def make_group(rng, variants_mod, overhang, use_affine):
    L = rng.randint(300, 1500)
    ref = list(rand_seq(rng, L))
    for _ in range(rng.randint(0, 4)):   # lower case and N stretches
        p = rng.randint(0, L - 10)
        for x in range(p, p + rng.randint(1, 8)):
            ref[x] = ref[x].lower() if rng.random() < 0.5 else "N"
    ref = "".join(ref)
    vs, pos = [], rng.randint(0, 30)
    while pos < L - 40:
        r = rng.random()
        if r < 0.55:
            v = Var(pos, ref[pos], [rng.choice([c for c in "ACGT" if c != ref[pos].upper()])])
        elif r < 0.68:
            k = rng.randint(1, 30)
            v = Var(pos, ref[pos], [ref[pos] + rand_seq(rng, k)])
        elif r < 0.8:
            k = rng.randint(1, 30)
            v = Var(pos, ref[pos:pos + k + 1], [ref[pos]])
        elif r < 0.87:
            k = rng.randint(2, 4)
            v = Var(pos, ref[pos:pos + k], [rand_seq(rng, k)])
        elif r < 0.95:
            v = Var(pos, ref[pos], [c for c in "ACGT" if c != ref[pos].upper()][:rng.randint(2, 3)] + ([ref[pos] + "AT"] if rng.random() < 0.5 else []))
        else:
            v = Var(pos, ref[pos], ["<DEL>"])
        vs.append(v)
        if rng.random() < 0.08:   # a second variant at the same position
            vs.append(Var(pos, ref[pos], [rng.choice("ACGT")]))
        pos += rng.randint(1, 40)
    restricted = None
    if rng.random() < 0.4:
        restricted = []
        for v in vs:
            k = len(v.get_alt_allele_list())
            choice = rng.random()
            restricted.append(Gt([0, 1]) if choice < 0.4 else Gt([1, 1]) if choice < 0.55 else Gt([0, 0]) if choice < 0.7 else
                              Gt(sorted(rng.sample(range(k + 1), min(k + 1, 2)))) if choice < 0.9 else Gt([0, k, 5]))
    reads = []
    for _ in range(rng.randint(3, 12)):
        start = rng.randint(0, L - 60)
        cigar, seq, rp = [], [], start
        if rng.random() < 0.3:
            n = rng.randint(1, 6)
            cigar.append((4, n))
            seq.append(rand_seq(rng, n))
        if rng.random() < 0.1:
            cigar.insert(0, (5, rng.randint(1, 5)))
        while rp < min(L, start + rng.randint(20, 400)):
            op = rng.choices([0, 1, 2, 3, 7, 8, 6], weights=[60, 8, 8, 2, 5, 5, 1])[0]
            n = rng.randint(1, 30) if op in (0, 7, 8) else rng.randint(1, 8)
            if op in (0, 7, 8, 2, 3):
                n = min(n, L - rp)
                if n <= 0:
                    break
            if op in (0, 7, 8):
                seg = list(ref[rp:rp + n])
                for x in range(len(seg)):
                    if rng.random() < 0.05:
                        seg[x] = rng.choice("ACGTN")
                seq.append("".join(seg))
                rp += n
            elif op == 1:
                seq.append(rand_seq(rng, n))
            elif op in (2, 3):
                rp += n
            cigar.append((op, n))
        if rng.random() < 0.2:
            n = rng.randint(1, 6)
            cigar.append((4, n))
            seq.append(rand_seq(rng, n))
        seq = "".join(seq)
        if rng.random() < 0.1:
            seq = seq[:rng.randint(0, len(seq))]   # CIGAR consumes more query than the sequence holds
        if rng.random() < 0.03:
            cigar = []
        j = 0
        while j < len(vs) and vs[j].position < start - rng.randint(0, 50):
            j += 1
        reads.append(Aln(start, cigar, seq))
        reads[-1].j = j
    kw = dict(overhang=overhang, use_affine=use_affine)
    if use_affine:
        kw.update(gap_start=rng.choice([1, 10]), gap_extend=rng.choice([1, 7]), default_mismatch=rng.choice([15.1, 0.3, 1, 20]))
    expected, errors = [], []
    R = variants_mod.ReadSetReader
    for a in reads:
        try:
            expected.append([list(t) for t in R.detect_alleles_by_alignment(vs, restricted, a.j, a, ref, **kw)])
        except (ValueError, AssertionError, IndexError, TypeError) as e:
            expected.append({"error": type(e).__name__})
    return {"reference": ref, "variants": [[v.position, v.reference_allele, v.get_alt_allele_list()] for v in vs],
            "restricted": None if restricted is None else [g.as_vector() for g in restricted],
            "reads": [{"start": a.reference_start, "cigar": [list(c) for c in a.cigartuples], "seq": a.query_sequence, "j": a.j} for a in reads],
            "params": kw, "expected": expected}


def make_error_groups(variants_mod):
    """Hand-made inputs for every exception realign raises."""
    ref = "ACGTACGTAC" * 8
    R = variants_mod.ReadSetReader
    cases = []
    def add(vs, restricted, reads, kw):
        exp = []
        for a in reads:
            try:
                exp.append([list(t) for t in R.detect_alleles_by_alignment(vs, restricted, a.j, a, ref, **kw)])
            except (ValueError, AssertionError, IndexError, TypeError) as e:
                exp.append({"error": type(e).__name__})
        cases.append({"reference": ref, "variants": [[v.position, v.reference_allele, v.get_alt_allele_list()] for v in vs],
                      "restricted": None if restricted is None else [g.as_vector() for g in restricted],
                      "reads": [{"start": a.reference_start, "cigar": [list(c) for c in a.cigartuples], "seq": a.query_sequence, "j": a.j} for a in reads],
                      "params": kw, "expected": exp})
    def aln(start, cigar, seq, j=0):
        a = Aln(start, cigar, seq)
        a.j = j
        return a
    v1 = [Var(30, "G", ["T"]), Var(40, "A", ["C"])]
    add(v1, None, [aln(20, [(0, 15), (9, 3), (0, 20)], ref[20:55])], dict(overhang=10))       # unsupported op
    add(v1, None, [aln(20, [(0, 5), (6, 2), (0, 30)], ref[20:55])], dict(overhang=10))        # P inside the left window
    add([Var(40, "A", ["C"]), Var(30, "G", ["T"])], None, [aln(20, [(0, 40)], ref[20:60])], dict(overhang=3))   # unsorted
    add(v1, [Gt([2, 3]), Gt([0, 1])], [aln(20, [(0, 40)], ref[20:60])], dict(overhang=3))      # empty allowed set
    add([Var(2, "G", ["T"])], None, [aln(0, [(0, 30)], ref[0:30])], dict(overhang=10))          # window left of the chromosome
    add([Var(75, "G", ["T"])], None, [aln(60, [(0, 20)], ref[60:80])], dict(overhang=10))       # window right of the chromosome
    add(v1, None, [aln(20, [(0, 40)], None)], dict(overhang=10))                                 # no query sequence
    add(v1, [Gt([1, 1]), Gt([0, 0, 1])], [aln(20, [(0, 40)], ref[20:60])], dict(overhang=3))  # duplicates in a restriction
    add(v1, None, [aln(30, [(0, 1), (0, 10)], ref[30:41]), aln(20, [(0, 11)], ref[20:31])], dict(overhang=10))   # variant at the first / last base
    return cases


def write_edge(align):
    """tests/golden/realign_edge_cases.json.gz: both distances of the reference for every pair of realign_cases.edge_pairs() -- the results
    and a hash of the generated inputs, no sequences."""
    sys.path.insert(0, os.path.dirname(HERE))
    import realign_cases

    pairs = realign_cases.edge_pairs()
    data = {"sha256": realign_cases.edge_hash(pairs), "n": len(pairs),
            "unit": [align.edit_distance(p["q"], p["t"]) for p in pairs],
            "affine": [align.edit_distance_affine_gap(p["q"], p["t"], p["costs"], p["gap"][0], p["gap"][1]) for p in pairs]}
    with open(OUT_EDGE, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0) as f:   # (no time stamp: the same bytes on every run)
        f.write(json.dumps(data, separators=(",", ":")).encode())
    print(f"{OUT_EDGE}: {len(pairs)} pairs, {os.path.getsize(OUT_EDGE)} bytes")


def main():
    args = [a for a in sys.argv[1:] if a != "--edge-only"]
    edge_only = len(args) != len(sys.argv) - 1   # --edge-only: leave realign_cases.json.gz as it is
    ref_root = args[0] if args else os.environ.get("WHATSHAP_REFERENCE", "/root/reference")
    if not os.path.isdir(os.path.join(ref_root, "whatshap")):
        sys.exit(f"no reference tree at {ref_root}")
    tmp = tempfile.mkdtemp(prefix="realign_ref_")
    try:
        align, variants_mod = build_reference(ref_root, tmp)
        write_edge(align)
        if edge_only:
            return
        rng = random.Random(20261015)
        pairs = make_pairs(rng, align)
        groups = []
        for overhang in (3, 10, 25):
            for use_affine in (False, True):
                for _ in range(12):
                    groups.append(make_group(rng, variants_mod, overhang, use_affine))
        groups += make_error_groups(variants_mod)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    with gzip.open(OUT, "wt") as f:
        json.dump({"pairs": pairs, "groups": groups}, f, separators=(",", ":"))
    n_reads = sum(len(g["reads"]) for g in groups)
    n_yields = sum(len(e) for g in groups for e in g["expected"] if isinstance(e, list))
    n_err = sum(1 for g in groups for e in g["expected"] if isinstance(e, dict))
    print(f"{OUT}: {len(pairs)} pairs, {len(groups)} groups, {n_reads} reads, {n_yields} yields, {n_err} errors")


if __name__ == "__main__":
    main()
