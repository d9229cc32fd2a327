"""Cases of the progeny genotype likelihoods (whatshap_amd.progeny: get_offspring_gl, compute_gt_likelihoods, correct_variant_types and the
array-level calls under them): the seeded generators of their inputs -- small stand-ins for the reference's variant tables and its
VariantInfo --, the loader of what the reference recorded for them (tests/golden/progeny_gl_cases.json.gz, written by
tests/golden/make_progeny_gl_golden.py), the exact rational value of a cell and the error bound of the device's arithmetic.

Inputs are generated, not stored: every number comes from Python's ``random.Random(seed)``, and the golden file keeps a SHA-256 over the
generated inputs of every case, so a drifting generator is noticed before any likelihood is compared.
"""
import base64
import decimal
import gzip
import hashlib
import json
import os
import random
import types
from fractions import Fraction

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "progeny_gl_cases.json.gz")

SN, DN, S2 = (1, 0), (2, 0), (1, 1)
U = Fraction(1, 2 ** 53)
CUTOFF = Fraction(1, 2 ** 999)   # a weight 1000 binades below the largest counts 0: the value it would have had is below this


# ---------------------------------------------------------------------------------------------- stand-ins for the reference's objects
class Table:
    """What get_offspring_gl asks of a VariantTable: len, variants[i].position, allele_depths_of(sample)."""

    class _Variant:
        def __init__(self, position):
            self.position = position

    def __init__(self, positions, depths=None):
        self.variants = [self._Variant(p) for p in positions]
        self._depths = depths or {}

    def __len__(self):
        return len(self.variants)

    def allele_depths_of(self, sample):
        return self._depths[sample]


class VariantInfo:
    """A minimal stand-in with the interface the scoring stage uses of the reference's VariantInfo: indexing gives a record with ref, alt,
    alt_count, co_alt_count; a variant is phasable when it has an alt allele, is not skipped and its type is one of the allowed ones;
    every phasable variant has alt_count nodes, in variant order; correct_type sets the type and takes the variant out of the phasable
    set when the type changed to one that cannot follow the old one."""

    MAY_FOLLOW = {SN: {SN, S2, DN}, S2: {S2}, DN: {SN, S2, DN}}

    def __init__(self, allowed_types):
        self._allowed = {tuple(t) for t in allowed_types}
        self._records = []
        self._phasable = []   # one flag per variant

    def __len__(self):
        return len(self._records)

    def __getitem__(self, variant):
        return self._records[variant]

    def append(self, ref, alt, alt_count, co_alt_count, skip=False):
        self._records.append(types.SimpleNamespace(ref=ref, alt=alt, alt_count=alt_count, co_alt_count=co_alt_count))
        self._phasable.append(alt is not None and not skip and (alt_count, co_alt_count) in self._allowed)

    def get_phasable(self):
        return [v for v, flag in enumerate(self._phasable) if flag]

    def remove_phasable(self, variant):
        assert self._phasable[variant], f"variant {variant} is not phasable"
        self._phasable[variant] = False

    def get_node_positions(self):
        return [v for v in self.get_phasable() for _ in range(self._records[v].alt_count)]

    def node_to_variant(self, node):
        return self.get_node_positions()[node]

    def correct_type(self, variant, alt_count, co_alt_count):
        record = self._records[variant]
        old, new = (record.alt_count, record.co_alt_count), (alt_count, co_alt_count)
        record.alt_count, record.co_alt_count = new
        if new != old and new not in self.MAY_FOLLOW.get(old, ()):
            self.remove_phasable(variant)


class Param:
    def __init__(self, ploidy, allele_error_rate, scoring_window=250):
        self.ploidy, self.allele_error_rate, self.scoring_window = ploidy, allele_error_rate, scoring_window


def state_of(varinfo):
    """What a call leaves behind in a VariantInfo: the phasable set and every variant's type."""
    return dict(phasable=[int(p) for p in varinfo.get_phasable()], alt=[int(varinfo[v].alt_count) for v in range(len(varinfo))],
                co=[int(varinfo[v].co_alt_count) for v in range(len(varinfo))])


# ---------------------------------------------------------------------------------------------- the recorded cases
def specs():
    out = []

    def add(name, ploidy, n_samples, n_variants, error_rate=0.06, max_depth=120, **kw):
        out.append(dict(name=name, ploidy=ploidy, n_samples=n_samples, n_variants=n_variants, error_rate=error_rate, max_depth=max_depth,
                        seed=kw.pop("seed", len(out) + 1), p_absent=kw.pop("p_absent", 0.1), p_same_position=kw.pop("p_same_position", 0.0),
                        p_short=kw.pop("p_short", 0.05), zero_position=kw.pop("zero_position", False),
                        progeny_duplicates=kw.pop("progeny_duplicates", False)))
        assert not kw

    add("p2", 2, 7, 30)
    add("p3", 3, 6, 24, error_rate=0.01)
    add("p4", 4, 12, 60, zero_position=True)
    add("p4_same_position", 4, 6, 40, p_same_position=0.3, progeny_duplicates=True)   # records of one position: the later nodes reuse the first's row
    add("p4_shallow", 4, 6, 24, max_depth=9, p_short=0.3)                                # many cells below the ploidy, short depth tuples
    add("p4_noisy", 4, 4, 20, error_rate=0.2)
    add("p6", 6, 6, 30)
    add("p8", 8, 5, 20, error_rate=0.03)
    add("nothing_phasable", 4, 3, 6, p_absent=1.0)
    return out


def _types(ploidy):
    return [SN, S2] if ploidy < 4 else [SN, SN, DN, S2]


def hyp(k, N, M, n):
    from math import comb
    return comb(M, k) * comb(N - M, n - k) / comb(N, n) if 0 <= k <= M and 0 <= n - k <= N - M else 0.0


def prior_row(ploidy, i, j):
    """compute_gt_likelihood_priors(ploidy)[i][j] (only used to draw genotypes for the generated depths)."""
    k = ploidy
    return [sum(hyp(l, k, i, k // 2) * hyp(m - l, k, j, k // 2) for l in range(m + 1)) for m in range(k + 1)]


class Case:
    """The generated inputs of a spec.  varinfo() makes a fresh VariantInfo (of ``cls``: the stand-in above, or the reference's own class
    at generation time), since the calls under test change it."""

    def __init__(self, spec):
        self.spec = spec
        rng = random.Random(spec["seed"] * 104729 + 7)
        k = spec["ploidy"]
        self.param = Param(k, spec["error_rate"])
        self.offspring = [f"progeny{s}" for s in range(spec["n_samples"])]
        # the parent's variants
        self.variants = []   # (position, ref, alt, alt_count, co_alt_count, skip)
        position = 0 if spec["zero_position"] else 100
        for v in range(spec["n_variants"]):
            if v and rng.random() >= spec["p_same_position"]:
                position += rng.randrange(1, 400)
            r = rng.random()
            if r < 0.08:
                self.variants.append((position, None, None, 0, 0, False))          # no genotype
            elif r < 0.14:
                self.variants.append((position, 0, None, 0, 0, False))             # homozygous
            else:
                ref, alt = rng.choice([(0, 1)] * 5 + [(1, 0), (0, 2), (2, 1)])
                t = rng.choice(_types(k) + [(3, 0)] * (k >= 6))
                self.variants.append((position, ref, alt, t[0], t[1], rng.random() < 0.05))
        self.variant_table = Table([v[0] for v in self.variants])
        # the progeny table: most of the parent's positions, some of its own, optionally records that repeat a position
        records = []   # (sort key, position, the variant it belongs to or None)
        seen = set()
        for v, var in enumerate(self.variants):
            if var[0] in seen or rng.random() < spec["p_absent"]:
                continue
            seen.add(var[0])
            records.append((var[0], var[0], v))
            if spec["progeny_duplicates"] and rng.random() < 0.15:
                records.append((var[0], var[0], v))
            if rng.random() < 0.2:
                records.append((var[0] + 0.5, 10_000_000 + v, None))   # a position of its own
        records.sort(key=lambda r: r[0])
        positions = [r[1] for r in records]
        depths = {}
        for sample in self.offspring:
            rows = []
            for _, _, v in records:
                if v is None or self.variants[v][2] is None:
                    rows.append((rng.randrange(40), rng.randrange(40)))
                    continue
                _, ref, alt, a, c, _ = self.variants[v]
                g = rng.choices(range(k + 1), weights=prior_row(k, min(a, k), min(c, k)))[0]
                u = rng.random()
                n = rng.randrange(k) if u < 0.08 else rng.randrange(k, k + 3) if u < 0.16 else rng.randrange(spec["max_depth"] + 1)
                p_alt = (1 - g / k) * spec["error_rate"] + (g / k) * (1 - spec["error_rate"])
                n_alt = sum(1 for _ in range(n) if rng.random() < p_alt)
                row = [rng.randrange(3), rng.randrange(3), rng.randrange(3)]
                row[ref], row[alt] = n - n_alt, n_alt
                if rng.random() < spec["p_short"]:
                    row = row[:rng.randrange(3)]
                elif max(ref, alt) < 2 and rng.random() < 0.5:
                    row = row[:2]
                rows.append(tuple(row))
            depths[sample] = rows
        self.progeny_table = Table(positions, depths)

    def varinfo(self, cls=VariantInfo):
        info = cls([SN, DN, S2])
        for _, ref, alt, a, c, skip in self.variants:
            info.append(ref, alt, a, c, skip)
        return info

    def sha256(self):
        blob = json.dumps([self.variants, [v.position for v in self.progeny_table.variants],
                           [self.progeny_table.allele_depths_of(s) for s in self.offspring]], separators=(",", ":"))
        return hashlib.sha256(blob.encode()).hexdigest()


# ---------------------------------------------------------------------------------------------- the golden file
def load_golden():
    with gzip.open(GOLDEN, "rt") as f:
        return json.load(f)


def unpack(b64, dtype):
    return np.frombuffer(base64.b64decode(b64), dtype=dtype)


def pack(arr, dtype):
    return base64.b64encode(np.ascontiguousarray(arr, dtype=dtype).tobytes()).decode("ascii")


# ---------------------------------------------------------------------------------------------- exact values and the bound
def alt_probability(g, ploidy, error_rate):
    """p_g as the reference forms it, in double (Python floats: the same operations in the same order)."""
    return (1 - g / ploidy) * error_rate + (g / ploidy) * (1 - error_rate)


def exact_cell(ref_dp, alt_dp, ploidy, error_rate, prior=None):
    """The exact rational likelihoods of one cell with data, from the doubles p_g, 1.0 - p_g and prior[g]."""
    w = []
    for g in range(ploidy + 1):
        p = alt_probability(g, ploidy, error_rate)
        w.append(Fraction(p) ** alt_dp * Fraction(1.0 - p) ** ref_dp * (Fraction(prior[g]) if prior is not None else 1))
    total = sum(w)
    return [x / total for x in w]


DECIMAL = decimal.Context(prec=120, Emin=decimal.MIN_EMIN, Emax=decimal.MAX_EMAX)


def decimal_cell(ref_dp, alt_dp, ploidy, error_rate, prior=None):
    """exact_cell for depths at which rationals are out of reach (a power of 100 000 has millions of digits): the same expression from
    the same doubles in 120-digit decimal arithmetic with an unbounded exponent.  Each of its 2 (k + 1) powers and 3 (k + 1) + k other
    operations is rounded to 120 digits, so its relative error stays below 1e-115 -- nothing against a bound of 1e-16 and more."""
    D = decimal.Decimal
    w = []
    for g in range(ploidy + 1):
        p = alt_probability(g, ploidy, error_rate)
        x = DECIMAL.multiply(DECIMAL.power(D(p), alt_dp), DECIMAL.power(D(1.0 - p), ref_dp))
        w.append(DECIMAL.multiply(x, D(prior[g])) if prior is not None else x)
    total = D(0)
    for x in w:
        total = DECIMAL.add(total, x)
    return [DECIMAL.divide(x, total) for x in w]


def bound(n, ploidy):
    """B(n, k): the relative error of the (mantissa, exponent) product form against the exact value, u = 2^-53.
    A power x^d taken by squaring is a product of d factors x: however the squarings group them, every rounding error enters once per
    factor it covers, d - 1 in total, so x^d carries (1 + e)^(d - 1), |e| <= u.  A weight is p^alt_dp * q^ref_dp * prior: (alt_dp - 1) +
    (ref_dp - 1) + 2 <= n roundings (frexp and ldexp are exact; the rebased weights are normal numbers since those 1000 binades below
    the largest are dropped).  The sum of the k + 1 non-negative weights adds at most k roundings to each, so it lies within
    (1 +- u)^(n + k) of the exact sum; the division adds one.  Together: |gl - exact| <= gamma(2n + k + 1) * exact with
    gamma(m) = m u / (1 - m u) -- of the order (n + k) 2^-53, 2.7e-14 at depth 120.  A dropped weight would have given a value below 2^-999:
    that absolute term (CUTOFF) is added where values are compared."""
    m = 2 * n + ploidy + 1
    return m * U / (1 - m * U)


# ---------------------------------------------------------------------------------------------- cells checked against exact values (host twin and device)
SHALLOW = (0, 1, 63, 64, 65)
UNDERFLOWING = [(61_000, 39_000), (39_000, 61_000), (90_000, 10_000)]   # between two genotypes' allele fractions: every pmf of the reference is 0
DEEP = [(100_000, 3), (3, 100_000), (50_000, 50_000), (2 ** 31 - 1, 5), (7, 2 ** 31 - 1)] + UNDERFLOWING
PRIOR_TYPES = {"none": None, "simplex_nulliplex": (1, 0), "duplex_nulliplex": (2, 0), "simplex_simplex": (1, 1), "nulliplex": (0, 0)}


def exact_problem(ploidy, prior_type):
    """One sample; rows: every pair of the depths 0, k - 1, k, 1, 63, 64, 65, then the deep cells."""
    from whatshap_amd import progeny

    depths = sorted(set(SHALLOW) | {ploidy - 1, ploidy})
    cells = [(r, a) for r in depths for a in depths] + DEEP
    kw = {}
    if prior_type is not None:
        kw = dict(priors=progeny.compute_gt_likelihood_priors(ploidy), row_alt_count=[prior_type[0]] * len(cells), row_co_alt_count=[prior_type[1]] * len(cells))
    return cells, progeny.DepthProblem([[c[0] for c in cells]], [[c[1] for c in cells]], ploidy, 0.06, **kw)


def check_exact(cells, problem, f64, table):
    """The doubles of every cell against the exact value -- rationals up to depth 130, 120-digit decimals beyond --, within B * exact (+ the
    cutoff's 2^-999); a deep cell is finite and sums to 1 within (k + 1) 2^-53."""
    k = problem.ploidy
    for row, (ref_dp, alt_dp) in enumerate(cells):
        got = f64[row, 0]
        if ref_dp + alt_dp < k:
            assert (got == -1.0).all() and (table[row, 0] == -1.0).all()
            continue
        prior = None if problem.priors is None else problem.priors[problem.row_alt_count[row], problem.row_co_alt_count[row]].tolist()
        deep = ref_dp + alt_dp > 130
        B = bound(ref_dp + alt_dp, k)
        if deep:
            assert np.isfinite(got).all() and abs(Fraction(sum(Fraction(float(x)) for x in got)) - 1) <= (k + 1) * U
            exact = decimal_cell(ref_dp, alt_dp, k, problem.error_rate, prior)
            for g in range(k + 1):
                slack = decimal.Decimal(B.numerator) / decimal.Decimal(B.denominator) * exact[g] + decimal.Decimal(2) ** -999
                assert abs(decimal.Decimal(float(got[g])) - exact[g]) <= slack, (ref_dp, alt_dp, g)
        else:
            exact = exact_cell(ref_dp, alt_dp, k, problem.error_rate, prior)
            for g in range(k + 1):
                assert abs(Fraction(float(got[g])) - exact[g]) <= B * exact[g] + CUTOFF, (ref_dp, alt_dp, g)
        assert np.array_equal(got.astype(np.float32), table[row, 0])


# ---------------------------------------------------------------------------------------------- the large problem (GPU tests, benchmark)
def large_depths(alt_count, co_alt_count, n_samples=200, ploidy=4, error_rate=0.06, mean_depth=30.0, seed=5):
    """(ref_depth, alt_depth) uint32 [n_samples][n_variants] for variants of the given parental types: per sample a genotype drawn from
    the type's prior, a Poisson read depth and a binomial alt count with errors.  numpy's generator: compared with the host twin and
    with the unfused path, not recorded."""
    rng = np.random.default_rng(seed)
    alt_count = np.asarray(alt_count)
    co_alt_count = np.asarray(co_alt_count)
    genotype = np.zeros((n_samples, alt_count.size), dtype=np.int64)
    for t in {(int(a), int(c)) for a, c in zip(alt_count, co_alt_count)}:
        pick = np.nonzero((alt_count == t[0]) & (co_alt_count == t[1]))[0]
        genotype[:, pick] = rng.choice(ploidy + 1, size=(n_samples, pick.size), p=prior_row(ploidy, *t))
    depth = rng.poisson(mean_depth, size=genotype.shape)
    f = genotype / ploidy
    alt = rng.binomial(depth, (1 - f) * error_rate + f * (1 - error_rate))
    return (depth - alt).astype(np.uint32), alt.astype(np.uint32)


class LargeTables:
    """The first variants of the large problem behind the stand-in tables (for timing the reference's own loop)."""

    def __init__(self, node_variant, alt_count, co_alt_count, ref, alt, ploidy, error_rate):
        n_var = int(node_variant[-1]) + 1
        self.types = [(int(alt_count[v]), int(co_alt_count[v])) for v in range(n_var)]
        self.offspring = [f"progeny{s}" for s in range(ref.shape[0])]
        self.param = Param(ploidy, error_rate)
        self.variant_table = Table([100 + v for v in range(n_var)])
        self.progeny_table = Table([100 + v for v in range(n_var)],
                                   {name: list(zip(ref[s, :n_var].tolist(), alt[s, :n_var].tolist())) for s, name in enumerate(self.offspring)})

    def varinfo(self, cls=VariantInfo):
        info = cls([SN, DN, S2])
        for a, c in self.types:
            info.append(0, 1, a, c)
        return info


def large_tables(n_nodes, n_samples=200):
    import progeny_cases as pc

    _, node_variant, alt_count, co_alt_count, _ = pc.large_problem(n_nodes=n_nodes, n_samples=n_samples)
    ref, alt = large_depths(alt_count, co_alt_count, n_samples=n_samples)
    return LargeTables(node_variant, alt_count, co_alt_count, ref, alt, 4, 0.06)
