"""Recorded realign cases (tests/golden/realign_cases.json.gz) as duck-typed objects, and a plain Python restatement of both distances
(whatshap/align.pyx:16-196: unit Levenshtein; Gotoh in f32 through numpy float32 scalars) for inputs the reference never saw."""
import gzip
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "realign_cases.json.gz")


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
        self.reference_start, self.cigartuples, self.query_sequence = start, [tuple(c) for c in cigar], seq


def load():
    with gzip.open(GOLDEN, "rt") as f:
        return json.load(f)


def group_objects(g):
    variants = [Var(*v) for v in g["variants"]]
    restricted = None if g["restricted"] is None else [Gt(r) for r in g["restricted"]]
    reads = [Aln(r["start"], r["cigar"], r["seq"]) for r in g["reads"]]
    return variants, restricted, reads, [r["j"] for r in g["reads"]]


def unit_distance(s: bytes, t: bytes) -> int:
    m, n = len(s), len(t)
    prev = list(range(m + 1))
    for j in range(1, n + 1):
        cur = [j] + [0] * m
        for i in range(1, m + 1):
            cur[i] = min(prev[i - 1] + (s[i - 1] != t[j - 1]), prev[i] + 1, cur[i - 1] + 1)
        prev = cur
    return prev[m]


def affine_distance(q: bytes, t: bytes, costs, gap_start: int, gap_extend: int) -> int:
    f32 = np.float32
    m, n, len_p = len(q), len(t), 0
    while m > 0 and n > 0 and q[len_p] == t[len_p]:
        len_p += 1
        m -= 1
        n -= 1
    while m > 0 and n > 0 and q[len_p + m - 1] == t[len_p + n - 1]:
        m -= 1
        n -= 1
    inf = f32(2147483647)
    f = lambda l: f32(float(gap_start + (l - 1) * gap_extend))
    gs, ge = f32(gap_start), f32(gap_extend)
    a = [f32(0)] + [inf] * m
    b = [f32(0)] + [f(i) for i in range(1, m + 1)]
    c = [f32(0)] + [inf] * m
    for j in range(1, n + 1):
        pa, pb, pc = a[0], b[0], c[0]
        a[0], b[0], c[0] = inf, inf, f(j)
        for i in range(1, m + 1):
            mc = f32(0) if q[len_p + i - 1] == t[len_p + j - 1] else f32(costs[i - 1 + len_p])
            ca = f32(min(pa, pb, pc) + mc)
            cb = f32(min(a[i - 1] + gs, b[i - 1] + ge, c[i - 1] + gs))
            cc = f32(min(a[i] + gs, b[i] + gs, c[i] + ge))
            pa, pb, pc = a[i], b[i], c[i]
            a[i], b[i], c[i] = ca, cb, cc
    return int(min(a[m], b[m], c[m]))
