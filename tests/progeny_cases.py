"""Cases of progeny marker scoring (whatshap_amd.progeny): the seeded generators of their inputs, the loader of what the reference
recorded for them (tests/golden/progeny_cases.json.gz, written by tests/golden/make_progeny_golden.py) and a numpy restatement of the
reference's loop that derives, from the inputs alone, the stored entries, the row each of them reads, and the error bound of a score.

Inputs are generated, not stored (a 60 x 300 x 5 table alone is 360 KB of incompressible floats): every number comes from Python's
``random.Random(seed)``, whose ``random()`` stream is fixed across versions, and the golden file keeps the SHA-256 of every generated
table, so a drifting generator is noticed before any score is compared.
"""
import base64
import gzip
import hashlib
import json
import math
import os
import random

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "progeny_cases.json.gz")

SN, DN, S2 = (1, 0), (2, 0), (1, 1)
KIND_SN, KIND_S2, KIND_DN, KIND_INF = 0, 1, 2, 3
KIND_OF_TYPE = {SN: KIND_SN, DN: KIND_DN, S2: KIND_S2}


# ---------------------------------------------------------------------------------------------- pair-score cases
def pair_specs():
    """The recorded pair-score cases: name, ploidy, samples, scoring window, the variant types in node order, and what the table holds."""
    specs = []

    def add(name, ploidy, n_samples, window, types, **kw):
        specs.append(dict(name=name, ploidy=ploidy, n_samples=n_samples, window=window, types=[list(t) for t in types], seed=len(specs) + 1,
                          p_missing=kw.pop("p_missing", 0.1), p_zero=kw.pop("p_zero", 0.1), empty_rows=kw.pop("empty_rows", 0),
                          rows_beyond=kw.pop("rows_beyond", 0), distinct_duplex_rows=kw.pop("distinct_duplex_rows", False)))
        assert not kw

    def mixed(rng, n, p_dn=0.12, p_s2=0.12, lead=()):
        return list(lead) + [DN if (r := rng.random()) < p_dn else S2 if r < p_dn + p_s2 else SN for _ in range(n)]

    rng = random.Random(4711)
    for ploidy in (2, 3, 4, 6, 8):
        for window in (4, 7, 50, 250):
            n_var = {4: 14, 7: 25, 50: 60, 250: 40}[window]
            n_samples = rng.choice((1, 2, 5, 17, 40))
            add(f"mixed_p{ploidy}_w{window}", ploidy, n_samples, window, mixed(rng, n_var))
    # the reference's stride list raises for windows below 4 (strides[-1] of an empty list): recorded as such
    add("window_1", 4, 5, 1, mixed(rng, 10))
    add("window_2", 4, 5, 2, mixed(rng, 10))
    # multiplex variants in front (anchors that store -inf only; behind a simplex-nulliplex anchor they would have no score kind)
    add("multiplex_lead", 4, 12, 7, mixed(rng, 20, lead=[(3, 0), (4, 0), (2, 1), (3, 1)]))
    add("multiplex_only", 6, 9, 50, [(3, 0), (2, 1), (4, 0), (2, 0), (5, 0), (3, 2)])
    add("duplex_runs", 4, 30, 50, [SN, DN, DN, SN, SN, DN, SN, S2, DN, DN, DN, SN], distinct_duplex_rows=True)
    add("many_samples", 4, 300, 50, mixed(rng, 30), p_missing=0.15)
    add("all_data", 6, 60, 50, mixed(rng, 40), p_missing=0.0, p_zero=0.0)
    add("zeros", 4, 50, 7, mixed(rng, 30), p_zero=0.5)
    add("missing", 3, 50, 7, mixed(rng, 30), p_missing=0.6, empty_rows=5)
    add("rows_beyond_table", 4, 20, 7, mixed(rng, 25), rows_beyond=4)
    add("one_node", 4, 10, 250, [SN])
    add("no_nodes", 4, 10, 250, [])
    add("no_samples", 4, 0, 7, mixed(rng, 12))
    add("medium", 4, 100, 250, mixed(rng, 2650, p_dn=0.06, p_s2=0.05), p_missing=0.1, p_zero=0.03)
    return specs


def build_pair_case(spec):
    """(table float32 [n_positions][n_samples][ploidy + 1], node_variant, alt_count, co_alt_count) of a spec.  A variant with alt_count a
    takes a consecutive nodes; by default they share one row (as compute_gt_likelihoods fills them), with ``distinct_duplex_rows`` they
    do not (then a score stored again is visibly the earlier node's).  ``rows_beyond``: that many nodes at the end lie beyond the table's
    numPositions (the reference reads 0.0 there)."""
    rng = random.Random(spec["seed"] * 7919 + 13)
    types = [tuple(t) for t in spec["types"]]
    k1 = spec["ploidy"] + 1
    node_variant = [v for v, t in enumerate(types) for _ in range(t[0])]
    n_nodes, n_samples = len(node_variant), spec["n_samples"]
    n_positions = n_nodes - spec["rows_beyond"]
    table = np.full((n_nodes, n_samples, k1), -1.0, dtype=np.float32)
    empty = set(rng.sample(range(n_nodes), spec["empty_rows"])) if spec["empty_rows"] else set()
    for node in range(n_nodes):
        if node and node_variant[node] == node_variant[node - 1] and not spec["distinct_duplex_rows"]:
            table[node] = table[node - 1]
            continue
        if node in empty:
            continue
        for s in range(n_samples):
            if rng.random() < spec["p_missing"]:
                continue
            row = [rng.random() ** 3 for _ in range(k1)]
            total = sum(row)
            row = [x / total for x in row]
            for g in range(k1):
                if rng.random() < spec["p_zero"]:
                    row[g] = 0.0
            table[node, s] = row
    alt = np.array([t[0] for t in types], dtype=np.uint32)
    co = np.array([t[1] for t in types], dtype=np.uint32)
    return table[:n_positions].copy(), np.array(node_variant, dtype=np.uint32), alt, co


def table_sha256(table):
    return hashlib.sha256(np.ascontiguousarray(table, dtype=np.float32).tobytes()).hexdigest()


# ---------------------------------------------------------------------------------------------- variant-type cases
def type_specs():
    return [dict(name=f"types_p{p}", ploidy=p, n_samples=s, n_variants=v, seed=100 + p, depth=12.0, error_rate=0.06)
            for p, s, v in ((2, 60, 12), (3, 80, 12), (4, 120, 40), (6, 120, 40), (8, 150, 12))]


def _poisson(rng, lam):
    limit, k, prod = math.exp(-lam), 0, rng.random()
    while prod > limit:
        k += 1
        prod *= rng.random()
    return k


def _ipow(x, n):
    r = 1.0
    for _ in range(n):   # (products only: no libm in the generated tables)
        r *= x
    return r


def build_type_case(spec, priors):
    """Realistic likelihood rows for get_most_likely_variant_type: per variant a parental type, per sample a genotype drawn from the priors
    of that type, a Poisson read depth and binomial allele counts with errors; likelihoods are the binomial probabilities of the counts
    under each genotype, normalised (compute_gt_likelihoods without the prior factor); a depth below the ploidy leaves the sample without
    data.  Returns (table float32 [n_variants][n_samples][ploidy + 1], the true types)."""
    rng = random.Random(spec["seed"])
    k = spec["ploidy"]
    table = np.full((spec["n_variants"], spec["n_samples"], k + 1), -1.0, dtype=np.float32)
    truth = []
    for v in range(spec["n_variants"]):
        g0 = rng.randrange(k + 1)
        g1 = rng.randrange(g0 + 1)
        truth.append((g0, g1))
        prior = priors[g0][g1]
        for s in range(spec["n_samples"]):
            u, g, acc = rng.random(), 0, prior[0]
            while u > acc and g < k:
                g += 1
                acc += prior[g]
            depth = _poisson(rng, spec["depth"])
            p_alt = (1 - g / k) * spec["error_rate"] + (g / k) * (1 - spec["error_rate"])
            alt = sum(1 for _ in range(depth) if rng.random() < p_alt)
            if depth < k:
                continue
            gl = []
            for h in range(k + 1):
                p = (1 - h / k) * spec["error_rate"] + (h / k) * (1 - spec["error_rate"])
                gl.append(math.comb(depth, alt) * _ipow(p, alt) * _ipow(1 - p, depth - alt))
            total = sum(gl)
            table[v, s] = [x / total for x in gl]
    return table, truth


# ---------------------------------------------------------------------------------------------- the golden file
def load_golden():
    with gzip.open(GOLDEN, "rt") as f:
        return json.load(f)


def unpack(b64, dtype):
    return np.frombuffer(base64.b64decode(b64), dtype=dtype)


def pack(arr, dtype):
    return base64.b64encode(np.ascontiguousarray(arr, dtype=dtype).tobytes()).decode("ascii")


def entries_digest(i, j, f64, f32_bits):
    """SHA-256 over a complete entry list (i, j as uint32, the double scores' bits, the float scores' bits) in triangular order."""
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(i, dtype="<u4").tobytes())
    h.update(np.ascontiguousarray(j, dtype="<u4").tobytes())
    h.update(np.ascontiguousarray(f64, dtype="<f8").view("<u8").tobytes())
    h.update(np.ascontiguousarray(f32_bits, dtype="<u4").tobytes())
    return h.hexdigest()


class Param:
    def __init__(self, scoring_window):
        self.scoring_window = scoring_window


class VarInfo:
    """The two things get_variant_scoring asks of a VariantInfo."""

    class _T:
        def __init__(self, alt, co):
            self.alt_count, self.co_alt_count = int(alt), int(co)

    def __init__(self, node_variant, alt, co):
        self._nodes = [int(v) for v in node_variant]
        self._types = [self._T(a, c) for a, c in zip(alt, co)]

    def get_node_positions(self):
        return self._nodes[:]

    def node_to_variant(self, node):
        return self._nodes[node]

    def __getitem__(self, v):
        return self._types[v]


# ---------------------------------------------------------------------------------------------- numpy restatement
def strides_of(w):
    w3, w7, w13 = w // 4, w // 2, 3 * w // 4
    strides = [i for i in range(1, w3 + 1)]
    strides += [strides[-1] + 3 * i for i in range(1, w7 - w3 + 1)]
    strides += [strides[-1] + 7 * i for i in range(1, w13 - w7 + 1)]
    strides += [strides[-1] + 13 * i for i in range(1, w - w13 + 1)]
    return strides


def derive_entries(node_variant, alt, co, window):
    """The stored entries of get_variant_scoring from the inputs alone, in triangular order: (hi, lo, eff, kind, reused) -- anchor lo = i,
    partner hi = j, eff the partner node whose row the stored score was computed from, kind KIND_* (KIND_INF: both nodes of one variant)."""
    var = np.asarray(node_variant, dtype=np.int64)
    alt = np.asarray(alt, dtype=np.int64)
    co = np.asarray(co, dtype=np.int64)
    n = var.size
    kind_of_variant = np.full(alt.size, -1, dtype=np.int64)
    for t, kd in KIND_OF_TYPE.items():
        kind_of_variant[(alt == t[0]) & (co == t[1])] = kd
    anchor_sn = (alt[var] == 1) & (co[var] == 0) if n else np.zeros(0, dtype=bool)
    prev_var = np.full(n, -1, dtype=np.int64)
    prev_eff = np.zeros(n, dtype=np.int64)
    prev_kind = np.zeros(n, dtype=np.int64)
    parts = []
    for s in strides_of(window):
        if s >= n:
            break
        i = np.arange(n - s)
        j = i + s
        nj = var[j]
        same = nj == var[i]
        scored = ~same & anchor_sn[i]
        reuse = scored & (nj == prev_var[i])
        new = scored & ~reuse
        assert (kind_of_variant[nj[new]] >= 0).all(), "a partner type without a score kind"
        prev_var[i[new]] = nj[new]
        prev_eff[i[new]] = j[new]
        prev_kind[i[new]] = kind_of_variant[nj[new]]
        keep = same | scored
        eff = np.where(same, j, prev_eff[i])
        kind = np.where(same, KIND_INF, prev_kind[i])
        parts.append((j[keep], i[keep], eff[keep], kind[keep], reuse[keep]))
    if not parts:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z, z, z.astype(bool)
    hi, lo, eff, kind, reused = (np.concatenate(x) for x in zip(*parts))
    o = np.lexsort((lo, hi))
    return hi[o], lo[o], eff[o], kind[o], reused[o]


def weights(ploidy):
    """(same, diff) [3][6] by kind and the start value -- the reference's expressions in double (ploidy 2: the duplex weights are NaN / inf)."""
    k = np.float64(ploidy)
    with np.errstate(all="ignore"):
        same = np.zeros((3, 6))
        diff = np.zeros((3, 6))
        same[KIND_SN] = [0.5, 0, 0, 0.5, 0, 0]
        a, b = (k / 2 - 1) / (2 * (k - 1)), k / (4 * (k - 1))
        diff[KIND_SN] = [a, b, b, a, 0, 0]
        for w in (same, diff):
            sn = w[KIND_SN]
            w[KIND_S2] = [sn[0] / 2.0, sn[1] / 2.0, (sn[2] + sn[0]) / 2.0, (sn[3] + sn[1]) / 2.0, (sn[4] + sn[2]) / 2.0, (sn[5] + sn[3]) / 2.0]
        same[KIND_DN] = [a, 0, b, b, 0, a]
        c = (k / 2 - 2) * (k / 2 - 1) / (2 * (k - 1) * (k - 2))
        d = (k / 2) * (k / 2 - 1) / (2 * (k - 1) * (k - 2))
        e = (k / 2) * (k / 2 - 1) / (k - 1) * (k - 2)
        diff[KIND_DN] = [c, d, e, e, d, c]
    return same, diff, math.log(1.0 / (ploidy - 1))


_PAIRS = [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)]


def restate_scores(table, n_nodes, ploidy, lo, eff, kind, chunk=20000):
    """(score, n, S) per entry from the inputs alone: the double score of the reference's loop restated in numpy (products and sums rounded
    one by one, samples in order), the number n of samples that contribute to it and S = |log(1/(k-1))| + sum |log(cooccur / disjoint)| over
    them -- the quantities of the device test's error bound 2^-53 (2n + 8) S."""
    table = np.asarray(table, dtype=np.float32)
    n_samples = table.shape[1]
    rows = np.zeros((n_nodes, n_samples, 3), dtype=np.float64)   # nodes beyond the table read 0.0
    rows[: table.shape[0]] = table[:n_nodes, :, :3]
    same, diff, start = weights(ploidy)
    lo, eff, kind = (np.asarray(x, dtype=np.int64) for x in (lo, eff, kind))
    score = np.full(lo.size, -np.inf)
    n_out = np.zeros(lo.size, dtype=np.int64)
    s_out = np.zeros(lo.size)
    for b in range(0, lo.size, chunk):
        sl = slice(b, min(b + chunk, lo.size))
        kd = kind[sl]
        live = kd != KIND_INF
        if not live.any():
            continue
        kk = np.where(live, kd, 0)
        a, p = rows[lo[sl]], rows[eff[sl]]          # [E][S][3]
        with np.errstate(all="ignore"):
            cooc = np.zeros(a.shape[:2])
            disj = np.zeros(a.shape[:2])
            for c, (f, g) in enumerate(_PAIRS):
                gl = a[:, :, f] * p[:, :, g]
                skip = (kk == KIND_SN) & (c >= 4)       # simplex-nulliplex: 4 cases
                cooc = np.where(skip[:, None], cooc, cooc + gl * same[kk, c][:, None])
                disj = np.where(skip[:, None], disj, disj + gl * diff[kk, c][:, None])
            has = ~((a[:, :, 0] < 0.0) | (p[:, :, 0] < 0.0)) & (cooc * disj > 0)
            term = np.where(has, np.log(np.where(has, cooc / disj, 1.0)), 0.0)
        total = np.full(term.shape[0], start)
        for s in range(n_samples):                      # in sample order; adding 0.0 for a skipped sample changes nothing
            total = np.where(has[:, s], total + term[:, s], total)
        score[sl] = np.where(live, total, -np.inf)
        n_out[sl] = np.where(live, has.sum(axis=1), 0)
        s_out[sl] = np.where(live, abs(start) + np.abs(term).sum(axis=1), 0.0)
    return score, n_out, s_out


def restate_type_llh(table, priors, nodes=None):
    """(llh [n][T], n [n][T], S [n][T]): get_most_likely_variant_type's llh of every parental type restated in numpy, and the bound's n and S
    (the start value 1.0 included in S)."""
    table = np.asarray(table, dtype=np.float32).astype(np.float64)
    k1 = table.shape[2]
    if nodes is None:
        nodes = range(table.shape[0])
    types = [(g0, g1) for g0 in range(k1) for g1 in range(g0 + 1)]
    llh = np.zeros((len(nodes), len(types)))
    cnt = np.zeros((len(nodes), len(types)), dtype=np.int64)
    big = np.zeros((len(nodes), len(types)))
    for x, node in enumerate(nodes):
        rows = table[node] if node < table.shape[0] else np.zeros(table.shape[1:])
        have = ~(rows[:, 0] < 0.0)
        for t, (g0, g1) in enumerate(types):
            like = np.zeros(rows.shape[0])
            for g in range(k1):
                like = like + priors[g0][g1][g] * rows[:, g]
            total, mag = 1.0, 1.0
            for s in np.nonzero(have)[0]:
                if like[s] <= 0.0:
                    total -= math.inf
                else:
                    total += math.log(like[s])
                    mag += abs(math.log(like[s]))
            llh[x, t], cnt[x, t], big[x, t] = total, int(have.sum()), mag
    return llh, cnt, big


def bound(n, s):
    """|device - reference| <= 2^-53 (2n + 8) S: the arguments of log are bit-identical (no contraction); the device's log is specified to
    3 ulp, the host's is below 1 ulp -> 8 * 2^-53 relative per term; two recursive sums of n + 1 terms add 2n * 2^-53 * S."""
    return 2.0 ** -53 * (2 * np.asarray(n, dtype=np.float64) + 8) * np.asarray(s, dtype=np.float64)


# ---------------------------------------------------------------------------------------------- the large problem (GPU tests, benchmark)
def large_problem(n_nodes=60000, n_samples=200, ploidy=4, window=250, seed=5, p_missing=0.1, p_dn=0.03, p_s2=0.03):
    """(table, node_variant, alt, co, window): about n_nodes nodes, ~10 % of the samples without data per node, a few % duplex and
    simplex-simplex variants (a duplex variant's two nodes share one row).  numpy's generator: compared with the host twin, not recorded."""
    rng = np.random.default_rng(seed)
    r = rng.random(n_nodes)
    alt = np.where(r < p_dn, 2, 1).astype(np.uint32)
    co = np.where((r >= p_dn) & (r < p_dn + p_s2), 1, 0).astype(np.uint32)
    node_variant = np.repeat(np.arange(alt.size, dtype=np.uint32), alt)[:n_nodes]
    n_var = int(node_variant[-1]) + 1
    alt, co = alt[:n_var].copy(), co[:n_var].copy()
    alt[n_var - 1] = int((node_variant == n_var - 1).sum())   # a duplex variant cut by the end keeps one node: make its type match
    if alt[n_var - 1] == 1 and r[n_var - 1] < p_dn:
        co[n_var - 1] = 0
    per_variant = rng.random((n_var, n_samples, ploidy + 1), dtype=np.float32) ** 3
    per_variant /= per_variant.sum(axis=2, keepdims=True)
    per_variant[rng.random((n_var, n_samples)) < p_missing] = -1.0
    return np.ascontiguousarray(per_variant[node_variant]), node_variant, alt, co, window
