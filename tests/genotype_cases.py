"""Inputs of the genotyping tests: small random ReadSets + pedigrees with genotype priors, as flat ProblemArrays, and their
conversion into the reference's own objects."""
import numpy as np

from whatshap_amd import _native


def random_case(seed, n_variants=8, n_reads=10, max_len=5, mode="single", max_coverage=None, recomb=(1, 40), uniform_prior=False,
                phred=(1, 40), blank=0.15):
    """mode: single | trio | quartet.  Reads sorted by first position; positions 10, 20, ..."""
    rng = np.random.default_rng(seed)
    n_ind = {"single": 1, "trio": 3, "quartet": 4}[mode]
    triples = {"single": [], "trio": [(0, 1, 2)], "quartet": [(0, 1, 2), (0, 1, 3)]}[mode]
    reads = []
    cover = np.zeros(n_variants, dtype=int)
    for _ in range(n_reads):
        length = int(rng.integers(2, max_len + 1))
        start = int(rng.integers(0, n_variants - 1))
        idx = [v for v in range(start, min(n_variants, start + length)) if v == start or rng.random() >= blank]
        if len(idx) < 2:
            idx = [start, start + 1] if start + 1 < n_variants else [start - 1, start]
        lo, hi = idx[0], idx[-1]
        if max_coverage is not None and cover[lo:hi + 1].max() >= max_coverage:
            continue
        cover[lo:hi + 1] += 1
        reads.append((int(rng.integers(0, n_ind)), [(10 * (v + 1), int(rng.integers(0, 2)), int(rng.integers(phred[0], phred[1] + 1))) for v in idx]))
    reads.sort(key=lambda r: r[1][0][0])
    read_ptr, pos, alle, qual, samples = [0], [], [], [], []
    for sample, variants in reads:
        samples.append(sample)
        for p, a, q in variants:
            pos.append(p); alle.append(a); qual.append(q)
        read_ptr.append(len(pos))
    positions = np.arange(1, n_variants + 1, dtype=np.uint32) * 10
    if uniform_prior:
        gl = np.full((n_ind, n_variants, 3), 1.0 / 3.0)
    else:
        gl = rng.random((n_ind, n_variants, 3)) + 0.05
        gl /= gl.sum(axis=2, keepdims=True)
    recombcost = rng.integers(recomb[0], recomb[1] + 1, size=n_variants).astype(np.uint32)
    return _native.ProblemArrays(
        np.asarray(read_ptr, dtype=np.uint64), np.asarray(pos, dtype=np.int32), np.asarray(alle, dtype=np.uint8),
        np.asarray(qual, dtype=np.uint32), np.asarray(samples, dtype=np.int32), np.arange(n_ind, dtype=np.uint32),
        np.asarray(triples, dtype=np.uint32).reshape(-1), np.ones((n_ind, n_variants), dtype=np.uint8), gl, recombcost, positions, False,
        n_variants=n_variants)


def reference_likelihoods(problem, ref):
    """[individuals][columns][3] from the REAL whatshap.core.GenotypeDPTable (oracle/_ref/cy)."""
    rs = ref.ReadSet()
    ptr = problem.read_ptr
    for r in range(problem.n_reads):
        read = ref.Read(f"read{r}", 60, 0, int(problem.read_sample_id[r]))
        for i in range(int(ptr[r]), int(ptr[r + 1])):
            read.add_variant(int(problem.var_position[i]), int(problem.var_allele[i]), int(problem.var_quality[i]))
        rs.add(read)
    ids = ref.NumericSampleIds()
    individual_ids = [int(x) for x in problem.individual_id]
    for numeric in range(max(individual_ids) + 1):
        assert ids[str(numeric)] == numeric
    ped = ref.Pedigree(ids)
    n_ind, n_var = problem.n_individuals, problem.n_variants
    gl = problem.genotype_likelihoods.reshape(n_ind, n_var, 3)
    for i, numeric in enumerate(individual_ids):
        gts = [ref.Genotype([0, 1]) for _ in range(n_var)]
        gls = [ref.PhredGenotypeLikelihoods([float(x) for x in gl[i, v]]) for v in range(n_var)]
        ped.add_individual(str(numeric), gts, gls)
    for f, m, c in problem.triple_ids.reshape(-1, 3):
        ped.add_relationship(str(int(f)), str(int(m)), str(int(c)))
    positions = None if problem.positions is None else [int(p) for p in problem.positions]
    table = ref.GenotypeDPTable(ids, rs, [int(x) for x in problem.recombcost], ped, positions)
    n_cols = len(positions) if positions is not None else len(rs.get_positions())
    out = np.zeros((n_ind, n_cols, 3), dtype=np.float64)
    for i, numeric in enumerate(individual_ids):
        for c in range(n_cols):
            likelihoods = table.get_genotype_likelihoods(str(numeric), c)
            out[i, c, :] = [likelihoods[ref.Genotype(g)] for g in ([0, 0], [0, 1], [1, 1])]
    return out


def range_case(n_variants, coverage, step, error_rate, phred, seed, trio=False, quartet=False, priors="random"):
    """A synthetic block (whatshap_amd.synthetic.synthetic_block) as a genotyping problem whose f64 chains shrink fast.
    phred: None keeps the generator's qualities (U{5..40}), a number overwrites every quality with it.
    priors: "random" (non-uniform, as the long-table tests), "uniform" (1/3 each: what genotyping without priors passes), or "confident":
    (1e-30, 1e-30, 1 - 2e-30) towards a random genotype per individual and column -- non-zero, so no normaliser of the reference becomes 0;
    where every read disagrees with the prior a column costs pe^coverage for every bipartition."""
    from whatshap_amd.synthetic import synthetic_block

    b = synthetic_block(n_variants, coverage, seed=seed, step=step, error_rate=error_rate, trio=trio, quartet=quartet)
    quality = b.var_quality if phred is None else np.full(b.var_quality.shape, int(phred), dtype=np.uint32)
    rng = np.random.default_rng(seed)
    shape = (b.n_individuals, b.n_variants, 3)
    if priors == "random":
        gl = rng.random(shape) + 0.05
        gl /= gl.sum(axis=2, keepdims=True)
    elif priors == "uniform":
        gl = np.full(shape, 1.0 / 3.0)
    elif priors == "confident":
        gl = np.full(shape, 1e-30)
        np.put_along_axis(gl, rng.integers(0, 3, size=shape[:2])[:, :, None], 1.0 - 2e-30, axis=2)
    else:
        raise ValueError(priors)
    return _native.ProblemArrays(b.read_ptr, b.var_position, b.var_allele, quality, b.read_sample_id, b.individual_id, b.triple_ids,
                                 b.genotype.reshape(b.n_individuals, -1), gl, b.recombcost, b.positions, False, n_variants=b.n_variants)


# The inputs of the dynamic-range tests (test_genotype_range_host.py, test_gpu_genotype_range.py): name -> (regime, arguments of range_case).
# Regimes, by the restatement's per-column normalisers (the factor by which a chain that is not rescaled shrinks):
#   deep     one run of the longest kind alone shrinks the total by more than 1e-150;
#   chain    four such runs in a row shrink a chain below the smallest normal f64 (1e-308);
#   product  a chain stays normal over four runs, the product of the two chains (seven runs) does not;
#   inside   close to that, but inside: the table must stay on the run path;
#   priors   confident priors against the reads and, for comparison, uniform ones;
#   long     thousands of columns (too slow for the restatement: compared with the reference class only).
RANGE_CASES = {
    "deep_coverage6": ("deep", dict(n_variants=200, coverage=6, step=2, error_rate=0.25, phred=60, seed=11)),
    "deep_coverage8": ("deep", dict(n_variants=160, coverage=8, step=1, error_rate=0.25, phred=60, seed=12)),
    "chain_single": ("chain", dict(n_variants=200, coverage=6, step=2, error_rate=0.10, phred=40, seed=13)),
    "chain_trio": ("chain", dict(n_variants=160, coverage=5, step=2, error_rate=0.25, phred=60, seed=14, trio=True)),
    "product_step3": ("product", dict(n_variants=200, coverage=6, step=3, error_rate=0.05, phred=60, seed=23)),
    "hifi_phred93": ("product", dict(n_variants=420, coverage=6, step=2, error_rate=0.02, phred=93, seed=16)),
    "inside_generator": ("inside", dict(n_variants=420, coverage=6, step=2, error_rate=0.02, phred=None, seed=17)),
    "inside_quartet": ("inside", dict(n_variants=300, coverage=4, step=2, error_rate=0.02, phred=None, seed=18, quartet=True)),
    "confident_single": ("priors", dict(n_variants=120, coverage=6, step=2, error_rate=0.02, phred=40, seed=19, priors="confident")),
    "confident_trio": ("priors", dict(n_variants=120, coverage=5, step=2, error_rate=0.02, phred=40, seed=20, trio=True, priors="confident")),
    "uniform_single": ("priors", dict(n_variants=120, coverage=6, step=2, error_rate=0.02, phred=40, seed=19, priors="uniform")),
    "uniform_trio": ("priors", dict(n_variants=120, coverage=5, step=2, error_rate=0.02, phred=40, seed=20, trio=True, priors="uniform")),
    "long_single": ("long", dict(n_variants=3000, coverage=6, step=2, error_rate=0.02, phred=93, seed=21)),
    "long_trio": ("long", dict(n_variants=1200, coverage=5, step=2, error_rate=0.02, phred=60, seed=22, trio=True)),
}

# Which path the device takes, as test_genotype_range_host.exponent_model predicts it from the reference alone, for the two
# long tables from one run of the restatement that is too slow to repeat in every test session (True: the run path keeps the table).
RUN_PATH = {
    "deep_coverage6": False, "deep_coverage8": False, "chain_single": True, "chain_trio": True, "product_step3": True, "hifi_phred93": True,
    "inside_generator": True, "inside_quartet": True, "confident_single": False, "confident_trio": False, "uniform_single": True,
    "uniform_trio": True, "long_single": True, "long_trio": True,
}
