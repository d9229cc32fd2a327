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


# ------------------------------------------------------------------------------------------------- the edge pairs
# Seeded pairs at the lengths where the kernels change path (query words / strips of 64 rows, carry words of 64 columns, the three
# affine launch shapes).  tests/golden/make_realign_golden.py imports this generator and records the reference's two distances for every
# pair in tests/golden/realign_edge_cases.json.gz: results and a hash of the inputs only, no sequences.
EDGE_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "realign_edge_cases.json.gz")
EDGE_M = (1, 63, 64, 65, 127, 128, 129, 192, 193, 300)      # stripped query lengths of the main grid
EDGE_N = (1, 63, 64, 65, 127, 128, 129, 300)                # stripped target lengths of the main grid
SHAPE_N = (1364, 1365, 5460, 5461)                          # the last / first target length of each affine launch shape
SHAPE_M = (65, 129, 300)
EDGE_COSTS = (15.1, 0.3, 2.5)
EDGE_GAPS = ((10, 7), (1, 1))
HUGE_GAPS = ((16777217, 3), (16777219, 5))                  # f32 sums are no longer exact integers: the operation order shows


def _rand(rng, n, alphabet="ACGT"):
    return [rng.choice(alphabet) for _ in range(n)]


def _other(rng, c, alphabet="ACGT"):
    return rng.choice([x for x in alphabet if x != c])


def _resized_copy(rng, q, n):
    """A copy of q brought to length n (a window of it, or q with inserted runs) with a few substitutions."""
    t = list(q)
    if n <= len(t):
        k = rng.randint(0, len(t) - n)
        t = t[k:k + n]
    while len(t) < n:
        p = rng.randint(0, len(t))
        t[p:p] = _rand(rng, min(n - len(t), rng.randint(1, 12)))
    for _ in range(rng.randint(1, 2 + n // 16)):
        p = rng.randrange(n)
        t[p] = rng.choice("ACGT")
    return t


def _sprinkle(rng, s, what="NnacgtR"):
    for k in range(len(s)):
        if rng.random() < 0.12:
            s[k] = rng.choice(what)
    return s


def _pin_ends(rng, q, t):
    """First and last bytes of q and t differ: prefix and suffix stripping removes nothing."""
    if q[0] == t[0]:
        t[0] = _other(rng, q[0])
    if len(t) > 1 or len(q) > 1:
        if q[-1] == t[-1]:
            if len(t) > 1:
                t[-1] = _other(rng, q[-1])
            else:
                q[-1] = _other(rng, t[-1])
    assert q[0] != t[0] and q[-1] != t[-1]


def edge_pairs():
    """[{"name", "group", "q", "t", "costs", "gap"}]: the same list on every call."""
    import random

    rng = random.Random(20261020)
    out = []

    def add(group, name, q, t, gap):
        q, t = "".join(q), "".join(t)
        out.append({"name": name, "group": group, "q": q, "t": t, "costs": [rng.choice(EDGE_COSTS) for _ in q], "gap": list(gap)})

    # the main grid: m x n x (edited copy | unrelated | N and lower case in both)
    for m in EDGE_M:
        for n in EDGE_N:
            for variant in ("edit", "random", "nlower"):
                q = _rand(rng, m)
                t = _rand(rng, n) if variant == "random" else _resized_copy(rng, q, n)
                if variant == "nlower":
                    _sprinkle(rng, q)
                    _sprinkle(rng, t)
                    if n > 2:
                        t[n // 2] = "N"
                _pin_ends(rng, q, t)
                add("grid", f"grid-{variant}-m{m}-n{n}", q, t, EDGE_GAPS[len(out) % 2])
    # stripping: the unstripped query is longer than 64 (a long job), the stripped one is not
    pre, suf = _rand(rng, 40), _rand(rng, 30)
    for gap in EDGE_GAPS:
        x, y = _rand(rng, 10), _rand(rng, 12)
        _pin_ends(rng, x, y)
        add("strip", "strip-m10", pre + x + suf, pre + y + suf, gap)
        x, y = _rand(rng, 64), _rand(rng, 70)
        _pin_ends(rng, x, y)
        add("strip", "strip-m64", pre[:20] + x + suf[:10], pre[:20] + y + suf[:10], gap)
        add("strip", "strip-m0", pre + suf + pre, pre + suf + _rand(rng, 9) + pre, gap)
        add("strip", "strip-n0", pre + _rand(rng, 9) + suf, pre + suf, gap)
        add("strip", "strip-n0-long", pre + _rand(rng, 70) + suf, pre + suf, gap)
        same = _sprinkle(rng, _rand(rng, 100))
        add("strip", "strip-equal", same, list(same), gap)
    # the shape edges: the longest target of a call decides the launch shape of its long jobs
    for n in SHAPE_N:
        for m in SHAPE_M:
            for variant in ("window", "random"):
                t = _rand(rng, n)
                if variant == "window":
                    k = rng.randint(0, n - m)
                    q = t[k:k + m]
                    for _ in range(4):
                        q[rng.randrange(m)] = rng.choice("ACGTN")
                    if k + m + 7 < n:
                        t[k + m // 2] = "n"
                else:
                    q = _rand(rng, m)
                _pin_ends(rng, q, t)
                add("shape", f"shape-{variant}-m{m}-n{n}", q, t, EDGE_GAPS[len(out) % 2])
    q, t = _rand(rng, 64), _rand(rng, 5461)   # a short job with a long target: no scratch
    _pin_ends(rng, q, t)
    add("shape", "shape-short-m64-n5461", q, t, (10, 7))
    # gaps beyond 2^24
    for gap in HUGE_GAPS:
        for m, n in ((64, 65), (65, 70), (129, 127), (130, 300)):
            q = _rand(rng, m)
            t = _resized_copy(rng, q, n)
            _pin_ends(rng, q, t)
            add("gap", f"gap-m{m}-n{n}", q, t, gap)
    return out


def edge_hash(pairs) -> str:
    import hashlib

    return hashlib.sha256(json.dumps([[p["name"], p["q"], p["t"], p["costs"], p["gap"]] for p in pairs], separators=(",", ":")).encode()).hexdigest()


def load_edge():
    """(pairs, fixture): the generated pairs and the reference's recorded distances ({"sha256", "unit": [...], "affine": [...]})."""
    with gzip.open(EDGE_GOLDEN, "rt") as f:
        return edge_pairs(), json.load(f)


# ------------------------------------------------------------------------------------------------- detect cases at the launch shapes
DETECT_OVERHANG = 40          # an SNV job's query is 2 * 40 + 1 = 81 bytes: every job of these cases is a long job
DETECT_DELETIONS = (1364, 1365, 5460, 5461)   # max_target_long: the window of allele 0 (the reference allele) of the deletion
DETECT_INSERTIONS = (1400, 5500)              # inserted bases; max_target_long = 81 + that, the window of allele 1 (left | alt | right)


def _flip(c):
    return "T" if c != "T" else "A"


def detect_shape_case(kind, size, seed=31):
    """One indel whose longest allele window decides the launch shape, an SNV on each side, and three reads with a few sequencing errors
    inside the windows (so that stripping leaves the kernels work): one carries the reference, one the indel and the left SNV, one starts
    soft-clipped and carries the right SNV (and the reference over a deletion, the insertion over an insertion).
    kind "del": size is the reference allele's window; kind "ins": size is the number of inserted bases.
    Returns {"reference", "variants", "reads", "overhang", "alleles": per read [(variant, allele)], "n_jobs", "n_long", "max_target_long"}."""
    import random

    rng = random.Random(seed * 100003 + size)
    oh = DETECT_OVERHANG
    span = size - (2 * oh + 1) if kind == "del" else size
    dl = span if kind == "del" else 0
    ref = "".join(_rand(rng, dl + 1200))
    pos, s1, s2 = 500, 200, dl + 801
    errors = (pos - 10, pos + 3, pos + dl + 6)

    def body(a, b, edits):
        s = list(ref[a:b])
        for p in edits:
            if a <= p < b:
                s[p - a] = _flip(ref[p])
        return "".join(s)

    snv1, snv2 = Var(s1, ref[s1], [_flip(ref[s1])]), Var(s2, ref[s2], [_flip(ref[s2])])
    reads = [Aln(100, [(0, dl + 1000)], body(100, dl + 1100, errors))]
    if kind == "del":
        indel = Var(pos, ref[pos:pos + dl + 1], [ref[pos]])
        reads.append(Aln(100, [(0, 401), (2, dl), (0, 599)], body(100, 501, errors + (s1,)) + body(501 + dl, dl + 1100, errors)))
        reads.append(Aln(400, [(4, 20), (0, dl + 500)], "A" * 20 + body(400, dl + 900, errors + (s2,))))
        alleles = [[(0, 0), (1, 0), (2, 0)], [(0, 1), (1, 1), (2, 0)], [(1, 0), (2, 1)]]
        longest = dl + 2 * oh + 1
    else:
        ins = _rand(rng, span)
        indel = Var(pos, ref[pos], [ref[pos] + "".join(ins)])
        ins[span // 2] = _flip(ins[span // 2])   # one error inside the insertion
        ins = "".join(ins)
        reads.append(Aln(100, [(0, 401), (1, span), (0, 599)], body(100, 501, errors + (s1,)) + ins + body(501, 1100, errors)))
        reads.append(Aln(400, [(4, 20), (0, 101), (1, span), (0, 399)], "A" * 20 + body(400, 501, errors) + ins + body(501, 900, errors + (s2,))))
        alleles = [[(0, 0), (1, 0), (2, 0)], [(0, 1), (1, 1), (2, 0)], [(1, 1), (2, 1)]]
        longest = 2 * oh + 1 + span
    return {"reference": ref, "variants": [snv1, indel, snv2], "reads": reads, "overhang": oh, "alleles": alleles, "n_jobs": 8, "n_long": 8,
            "max_target_long": longest}


def reuse_pairs(n_pairs, waves, m_range, long_range, short_range, first_target, seed):
    """n_pairs (query, target, costs) with every query longer than 64 after stripping (ends differ) and target lengths that alternate long
    and short both along the pairs and along a grid-stride walk of `waves` rows: the row a job runs on was filled by a longer job before it,
    or by a shorter one.  Pair 0's target has first_target bytes (it sets the launch shape)."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    out = []
    for k in range(n_pairs):
        lo, hi = long_range if (k // waves + k) % 2 == 0 else short_range
        n = first_target if k == 0 else int(rng.integers(lo, hi + 1))
        m = int(rng.integers(m_range[0], m_range[1] + 1))
        ti = rng.integers(0, 4, n)
        if k % 3:   # related: the target's head (or all of it, padded) with a few substitutions
            qi = np.concatenate([ti[:m], rng.integers(0, 4, max(0, m - n))])
            qi[rng.integers(0, m, 3)] = rng.integers(0, 4, 3)
        else:
            qi = rng.integers(0, 4, m)
        if qi[0] == ti[0]:
            qi[0] = (qi[0] + 1) % 4
        if qi[-1] == ti[-1]:
            qi[-1] = (qi[-1] + 1) % 4
        costs = np.asarray(EDGE_COSTS)[rng.integers(0, 3, m)]
        out.append((acgt[qi].tobytes(), acgt[ti].tobytes(), costs))
    return out


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
