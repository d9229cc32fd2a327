"""Cases of the prior genotype likelihoods (whatshap_amd.genotype.compute_genotypes / prior_likelihoods): seeded generators, the array
form of a case, a plain-Python chain (IEEE doubles, no fused multiply-add, left-to-right sums) and the recorded reference results of
tests/golden/prior_genotype_cases.json.gz (written by tests/golden/make_prior_genotype_golden.py from the reference's own
compute_genotypes and its regularisation loop).

A case is a dict of plain lists: ``read_ptr``, ``pos``, ``allele``, ``qual`` (the reads as CSR), ``positions`` (list or None),
``constant`` and ``gt_qual_threshold`` (None: no regularisation recorded).  The golden file holds the cases themselves, so the tests
never depend on the generators staying as they are.
"""
import gzip
import json
import math
import os
import random

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prior_genotype_cases.json.gz")

QUALITIES = (0, 1, 5, 9, 13, 14, 20, 40, 93)
ALLELES = (0, 1, 2, 3)
CONSTANTS = (0.0, 1e-3, 0.5)
THRESHOLDS = (0, 10, 30)
# the device's classes (csrc/priorgt.h): each class's largest run and the next one's smallest; 4097 is one element beyond the tile the
# last class passes through LDS, 1025 one beyond what the LDS-resident class holds
BOUNDARY_RUNS = (1, 2, 7, 8, 9, 63, 64, 65, 1023, 1024, 1025, 4096, 4097)


# ---------------------------------------------------------------------------------------------- generators
def random_case(seed, name=None, positions_none=False, regularise=None):
    """At most 40 reads x 30 positions: listed positions nobody covers, entries at positions that are not listed, reads of one entry,
    many reads with the same first position, alleles 0 .. 3, the qualities on both sides of the 0.05 floor."""
    rng = random.Random(seed)
    n_universe = rng.randint(1, 24)
    universe = sorted(rng.sample(range(10, 400), n_universe))
    listed = [p for p in universe if rng.random() < 0.8] or [universe[0]]
    if positions_none:
        listed = list(universe)
    uncovered = [] if positions_none else rng.sample(range(400, 460), rng.randint(0, 6)) + rng.sample(range(0, 10), rng.randint(0, 2))
    in_list = set(listed)
    reads = []
    n_reads = rng.randint(0, 40)
    shared_start = rng.randrange(n_universe)
    for _ in range(n_reads):
        start = shared_start if rng.random() < 0.4 else rng.randrange(n_universe)
        length = 1 if rng.random() < 0.2 else rng.randint(1, 12)
        span = [p for p in universe[start:start + length] if rng.random() < 0.85]
        while span and span[0] not in in_list:
            span.pop(0)
        while span and span[-1] not in in_list:
            span.pop()
        if not span:
            continue
        reads.append([(p, rng.choice(ALLELES) if rng.random() < 0.3 else rng.choice((0, 1)), rng.choice(QUALITIES)) for p in span])
    reads.sort(key=lambda r: r[0][0])   # (stable: reads with the same first position keep their order)
    case = from_reads(name or f"random_{seed}", reads, None if positions_none else sorted(listed + uncovered))
    if regularise is not None:
        case["constant"], case["gt_qual_threshold"] = regularise
    return case


def from_reads(name, reads, positions, constant=None, gt_qual_threshold=None):
    read_ptr, pos, allele, qual = [0], [], [], []
    for read in reads:
        for p, a, q in read:
            pos.append(p)
            allele.append(a)
            qual.append(q)
        read_ptr.append(len(pos))
    return dict(name=name, read_ptr=read_ptr, pos=pos, allele=allele, qual=qual, positions=positions, constant=constant, gt_qual_threshold=gt_qual_threshold)


def run_case(n, name=None, position=100):
    """n single-entry reads on one position, every one counted: alleles and qualities mixed with period 7 and 9."""
    return from_reads(name or f"run_{n}", [[(position, (i % 7) & 1, QUALITIES[i % len(QUALITIES)])] for i in range(n)], [position])


def all_cases():
    cases = []
    for k in range(40):
        reg = (CONSTANTS[k % 3], THRESHOLDS[(k // 3) % 3]) if k % 2 == 0 else None
        cases.append(random_case(1000 + k, positions_none=(k % 5 == 4), regularise=reg))
    cases += [run_case(n) for n in BOUNDARY_RUNS]
    cases.append(from_reads("deep_ref_q30", [[(7, 0, 30)] for _ in range(1300)], [7]))
    cases.append(from_reads("no_reads", [], [3, 9, 27], constant=1e-3, gt_qual_threshold=10))
    cases.append(from_reads("no_positions", [], []))
    cases.append(from_reads("none_counted", [[(5, 2, 30), (8, 3, 20)], [(8, 2, 1)]], [5, 8, 11]))
    # the regularisation grid on one problem with an uncovered position (three equal values: the two largest tie) and a symmetric column
    grid_reads = [[(20, 0, 30), (30, 0, 20), (40, 1, 9)], [(20, 1, 30), (30, 0, 5), (40, 1, 13)], [(30, 0, 40)], [(40, 1, 93), (50, 0, 0)]]
    for c in CONSTANTS:
        for t in THRESHOLDS:
            cases.append(from_reads(f"grid_c{c}_t{t}", grid_reads, [20, 25, 30, 40, 50], constant=c, gt_qual_threshold=t))
    return cases


def fresh_batch(seed, n):
    """n small problems the reference was not run on (device against host twin)."""
    return [random_case(seed * 10_000 + k, positions_none=(k % 7 == 3), regularise=(CONSTANTS[k % 3], THRESHOLDS[k % 3]) if k % 2 else None) for k in range(n)]


# ---------------------------------------------------------------------------------------------- forms of a case
def problem_of(case):
    from whatshap_amd import genotype as gt

    reg = case["constant"] is not None
    return gt.PriorProblem(case["read_ptr"], case["pos"], case["allele"], case["qual"], case["positions"], constant=case["constant"] if reg else 0.0,
                           gt_prob=gt_prob_of(case) if reg else 0.0, want_regularized=reg)


def gt_prob_of(case):
    return 1.0 - (10 ** (-case["gt_qual_threshold"] / 10.0))


def readset_of(case, core):
    """The case as a ReadSet of `core` (whatshap_amd.core or the reference's whatshap.core)."""
    readset = core.ReadSet()
    ptr = case["read_ptr"]
    for r in range(len(ptr) - 1):
        read = core.Read(f"read{r}", 60, 0, 0)
        for x in range(ptr[r], ptr[r + 1]):
            read.add_variant(case["pos"][x], case["allele"][x], case["qual"][x])
        readset.add(read)
    return readset


def listed_positions(case):
    return sorted(set(case["pos"])) if case["positions"] is None else list(case["positions"])


def columns_of(case):
    """Per listed position the counted (allele, quality) pairs in read order."""
    index = {p: c for c, p in enumerate(listed_positions(case))}
    columns = [[] for _ in index]
    for p, a, q in zip(case["pos"], case["allele"], case["qual"]):
        if p in index and a in (0, 1):
            columns[index[p]].append((a, q))
    return columns


# ---------------------------------------------------------------------------------------------- the chain in plain Python
def python_chain(entries):
    """GenotypeDistribution's operator* over the entries in order, then normalize(): a 3-tuple."""
    d = [1.0 / 3.0, 1.0 / 3.0, 1.0 / 3.0]
    for allele, q in entries:
        p = max(0.05, math.pow(10.0, -float(q) / 10.0))
        f = (2.0 / 3.0 - 1.0 / 3.0 * p, 1.0 / 3.0, 1.0 / 3.0 * p)
        if allele == 1:
            f = f[::-1]
        d = [d[0] * f[0], d[1] * f[1], d[2] * f[2]]
        s = 0.0
        for x in d:
            s = s + x
        d = [x / s for x in d]
    s = 0.0
    for x in d:
        s = s + x
    if s <= 0.0:
        return (1.0 / 3.0, 1.0 / 3.0, 1.0 / 3.0)
    return tuple(x / s for x in d)


def python_genotype(gl):
    best_index, best = 0, 0.0
    for i in range(3):
        if gl[i] > best:
            best, best_index = gl[i], i
    err = 0.0
    for i in range(3):
        if i != best_index:
            err = err + gl[i]
    return best_index if err < 0.1 else -1


def hex3(values):
    return [float(v).hex() for v in values]


def load_golden():
    with gzip.open(GOLDEN, "rb") as f:
        return json.loads(f.read().decode())["cases"]
