"""GPU: the progeny genotype likelihoods on the device (progeny_gl_kernel) and the fused call from allele depths to scores.

The bound.  One cell is gl[g] = w_g / sum_g w_g with w_g = p_g^alt_dp * (1 - p_g)^ref_dp * prior[g]; u = 2^-53, n = ref_dp + alt_dp.
A power x^d taken by squaring on (mantissa, exponent) pairs is a product of d factors x: however the squarings group them, every
rounding error enters once per factor it covers, d - 1 in total (frexp and ldexp are exact).  A weight therefore carries
(alt_dp - 1) + (ref_dp - 1) + 2 <= n roundings; the sum of the k + 1 non-negative weights, rebased on the largest so that none is
subnormal, adds at most k to each; the division adds one:
    |gl - exact| <= B(n, k) * exact + 2^-999,   B(n, k) = gamma(2n + k + 1),   gamma(m) = m u / (1 - m u)
(progeny_gl_cases.bound) against the exact value of the doubles p_g, 1.0 - p_g and prior[g]; 2^-999 covers the weights dropped for lying
1000 binades or more below the largest.  Of the order (n + k) 2^-53: 2.7e-14 at depth 120.
Host and device run the same function, whose operations -- multiplications, additions, one division, frexp, ldexp, all without
contraction -- are correctly rounded on both: the device's doubles are the host twin's bit for bit, and the twin is tied to the reference by
tests/test_progeny_gl_host.py (float table bit-identical on every recorded case, doubles within B + E_ref)."""
import numpy as np
import pytest

import progeny_cases as pc
import progeny_gl_cases as gc
from whatshap_amd import progeny

pytestmark = pytest.mark.gpu

GOLD = gc.load_golden()
CASES = GOLD["cases"]
IDS = [c["spec"]["name"] for c in CASES]


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def recorded_problem(rec):
    case = gc.Case(rec["spec"])
    assert case.sha256() == rec["inputs_sha256"], "the case generator no longer produces the recorded inputs"
    return progeny.DepthProblem.from_tables(case.variant_table, case.progeny_table, case.offspring, case.varinfo(), case.param)


def both(problems):
    """(device tables, device doubles, twin tables, twin doubles) of a batch, one call each."""
    d64: list = []
    h64: list = []
    dev = progeny.offspring_gl_batch(problems, doubles=d64)
    host = progeny.offspring_gl_batch(problems, host=True, doubles=h64)
    return dev, d64, host, h64


def assert_equals_twin(problems):
    dev, d64, host, h64 = both(problems)
    for p, a, b, c, d in zip(problems, dev, d64, host, h64):
        assert a.array().shape == (p.n_nodes, p.n_samples, p.ploidy + 1)
        assert np.array_equal(bits64(b), bits64(d)) and np.array_equal(bits32(a.array()), bits32(c.array()))
    return dev


@pytest.fixture(scope="module")
def recorded():
    return [recorded_problem(rec) for rec in CASES]


@pytest.mark.parametrize("x", range(len(CASES)), ids=IDS)
def test_recorded_case(recorded, x):
    rec = CASES[x]
    table = assert_equals_twin([recorded[x]])[0]
    assert np.array_equal(bits32(table.array()).reshape(-1), gc.unpack(rec["f32_bits"], "<u4"))


def test_recorded_cases_as_one_batch(recorded):
    """Mixed ploidies in one launch."""
    assert len({p.ploidy for p in recorded}) >= 5
    for rec, table in zip(CASES, assert_equals_twin(recorded)):
        assert np.array_equal(bits32(table.array()).reshape(-1), gc.unpack(rec["f32_bits"], "<u4"))


# ---------------------------------------------------------------------------------------------- shapes
def synthetic(n_variants, n_samples, seed, ploidy=4, window=4, types=(gc.SN, gc.SN, gc.SN, gc.DN, gc.S2), error_rate=0.06, mean_depth=25.0):
    """A depth problem with scoring arrays: variants of random types, alt_count nodes each, one depth row per variant."""
    rng = np.random.default_rng(seed)
    t = np.array(types)[rng.integers(len(types), size=n_variants)].reshape(n_variants, 2)
    alt, co = t[:, 0].astype(np.uint32), t[:, 1].astype(np.uint32)
    ref_dp, alt_dp = gc.large_depths(alt, co, n_samples=n_samples, ploidy=ploidy, error_rate=error_rate, mean_depth=mean_depth, seed=seed)
    ref_dp[rng.random(ref_dp.shape) < 0.1] = 0   # some cells below the ploidy
    alt_dp[ref_dp == 0] = rng.integers(0, ploidy, size=int((ref_dp == 0).sum()))
    node_variant = np.repeat(np.arange(n_variants, dtype=np.uint32), alt)
    return progeny.DepthProblem(ref_dp, alt_dp, ploidy, error_rate, node_row=node_variant, priors=progeny.compute_gt_likelihood_priors(ploidy),
                                row_alt_count=alt, row_co_alt_count=co, node_variant=node_variant, alt_count=alt, co_alt_count=co, scoring_window=window)


def with_nodes(n_nodes, n_samples, seed, runs=()):
    """n_nodes simplex nodes, one row each, except the runs (first node, length) of nodes that share a row."""
    p = synthetic(n_nodes, n_samples, seed, types=(gc.SN,))
    node_row = np.arange(n_nodes, dtype=np.uint32)
    for first, length in runs:
        node_row[first:first + length] = first
    return progeny.DepthProblem(p.ref_depth, p.alt_depth, 4, 0.06, node_row=node_row, priors=p.priors, row_alt_count=p.row_alt_count,
                                row_co_alt_count=p.row_co_alt_count, node_variant=p.node_variant, alt_count=p.alt_count, co_alt_count=p.co_alt_count,
                                scoring_window=4)


def fused_and_unfused(problems):
    """(scores from depths, their stats, scores of score_variants_batch on the tables offspring_gl_batch downloaded)."""
    stats: list = []
    fused = progeny.score_variants_from_depths(problems, stats=stats)
    tables = progeny.offspring_gl_batch(problems)
    unfused = progeny.score_variants_batch([progeny.ProgenyProblem(t, p.node_variant, p.alt_count, p.co_alt_count, p.scoring_window)
                                            for t, p in zip(tables, problems)])
    return fused, stats, unfused


def assert_same_scores(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for u, v in zip(x.arrays(), y.arrays()):
            assert np.array_equal(u.view(np.uint32), v.view(np.uint32))
        assert np.array_equal(bits64(x.scores_f64()), bits64(y.scores_f64()))


@pytest.mark.parametrize("n_samples", (1, 3, 200))
@pytest.mark.parametrize("n_nodes", (1, 63, 64, 65, 257))
def test_shapes(n_nodes, n_samples):
    """Both lane orders: the full table against the twin, the planes through the scores they give."""
    p = with_nodes(n_nodes, n_samples, seed=n_nodes * 1000 + n_samples)
    assert_equals_twin([p])
    fused, stats, unfused = fused_and_unfused([p])
    assert_same_scores(fused, unfused)
    assert len(fused[0]) == sum(max(n_nodes - s, 0) for s in pc.strides_of(4)) and stats[0]["launches"] == (2 if n_nodes > 1 else 0)


def test_rows_shared_across_a_wave_boundary_and_an_empty_problem_inside_a_batch():
    shared = with_nodes(200, 5, seed=11, runs=((63, 2), (126, 3), (190, 3)))   # nodes 63-64 and 126-128 straddle lanes 64 and 128
    empty = progeny.DepthProblem(np.zeros((5, 0)), np.zeros((5, 0)), 6, 0.1, node_variant=[], alt_count=[], co_alt_count=[], scoring_window=4)
    batch = [with_nodes(65, 3, seed=12), empty, shared, synthetic(40, 7, seed=13, ploidy=6)]
    tables = assert_equals_twin(batch)
    t = tables[2].array()
    assert np.array_equal(t[63], t[64]) and np.array_equal(t[126], t[127]) and np.array_equal(t[126], t[128]) and not np.array_equal(t[62], t[63])
    assert tables[1].array().shape == (0, 5, 7)
    fused, _, unfused = fused_and_unfused(batch)
    assert_same_scores(fused, unfused)


def test_more_cells_than_one_grid_pass():
    """21 000 rows x 200 samples = 4.2 M cells, more than 16384 blocks x 256 lanes: the grid-stride loop wraps in either lane order.  The
    full table against the twin on the nodes at both ends (sample-fastest order: the wrapped cells are the last nodes') and on every 37th
    node in between, every row a distribution or without data; the planes (node-fastest order: the wrapped cells are the last sample's) through fused against unfused."""
    p = synthetic(21_000, 200, seed=21, types=(gc.SN,))
    assert p.n_nodes * p.n_samples > 16384 * 256
    d64: list = []
    table = progeny.offspring_gl_batch([p], doubles=d64)[0].array()
    for nodes in (np.arange(0, 300), np.arange(7, 21_000, 37), np.arange(20_700, 21_000)):
        sub = progeny.DepthProblem(p.ref_depth, p.alt_depth, 4, 0.06, node_row=p.node_row[nodes], priors=p.priors, row_alt_count=p.row_alt_count,
                                   row_co_alt_count=p.row_co_alt_count)
        h64: list = []
        host = progeny.offspring_gl_batch([sub], host=True, doubles=h64)[0].array()
        assert np.array_equal(bits32(table[nodes]), bits32(host)) and np.array_equal(bits64(d64[0][nodes]), bits64(h64[0]))
    total = d64[0].sum(axis=2)
    assert (((d64[0][:, :, 0] == -1.0) & (total == -5.0)) | (np.abs(total - 1.0) <= 2.0 ** -50)).all()   # (numpy's own summation included)
    fused, stats, unfused = fused_and_unfused([p])
    assert_same_scores(fused, unfused)
    assert stats[0]["launches"] == 2 and len(fused[0]) == sum(21_000 - s for s in pc.strides_of(4))


# ---------------------------------------------------------------------------------------------- deep cells
@pytest.mark.parametrize("prior", ("none", "simplex_nulliplex", "duplex_nulliplex"))
@pytest.mark.parametrize("ploidy", (2, 4, 8))
def test_deep_cells_against_exact_values(ploidy, prior):
    """Depths the reference cannot do, 2^31 - 1 on one side included, on the device against exact values (and the shallow edge depths)."""
    cells, problem = gc.exact_problem(ploidy, gc.PRIOR_TYPES[prior])
    d64: list = []
    table = progeny.offspring_gl_batch([problem], doubles=d64)[0]
    gc.check_exact(cells, problem, d64[0], table.array())


# ---------------------------------------------------------------------------------------------- fused against unfused
def fused_problems():
    return [synthetic(300, 40, seed=31, window=250), synthetic(500, 17, seed=32, window=4), synthetic(120, 200, seed=33, ploidy=6, window=50)]


def test_fused_equals_unfused():
    problems = fused_problems()
    kinds = set()
    for p in problems:
        kinds |= set(pc.derive_entries(p.node_variant, p.alt_count, p.co_alt_count, p.scoring_window)[3].tolist())
    assert kinds == {pc.KIND_SN, pc.KIND_S2, pc.KIND_DN, pc.KIND_INF}
    fused, stats, unfused = fused_and_unfused(problems)
    assert_same_scores(fused, unfused)
    for p, got, st in zip(problems, fused, stats):
        hi, lo, _, kind, reused = pc.derive_entries(p.node_variant, p.alt_count, p.co_alt_count, p.scoring_window)
        i, j, _ = got.arrays()
        assert np.array_equal(i, hi) and np.array_equal(j, lo) and np.isfinite(got.scores_f64()[kind != pc.KIND_INF]).all()
        assert st["launches"] == 2 and st["n_entries"] == hi.size and st["n_inf"] == int((kind == pc.KIND_INF).sum()) and st["n_reused"] == int(reused.sum())


def test_fused_is_deterministic():
    problems = fused_problems()
    assert_same_scores(progeny.score_variants_from_depths(problems), progeny.score_variants_from_depths(problems))
    a, b = progeny.offspring_gl_batch(problems), progeny.offspring_gl_batch(problems)
    assert all(np.array_equal(bits32(x.array()), bits32(y.array())) for x, y in zip(a, b))


def test_a_fused_call_without_samples_launches_the_pair_kernel_alone():
    """No sample, so no cell and no plane: the likelihood kernel is not launched, and every entry's score is the sum over no samples."""
    p = synthetic(12, 0, seed=51, types=(gc.SN,))
    assert p.n_samples == 0 and p.n_nodes == 12
    fused, stats, unfused = fused_and_unfused([p])
    assert_same_scores(fused, unfused)
    host = progeny.score_variants_batch([progeny.ProgenyProblem(progeny.offspring_gl_batch([p], host=True)[0], p.node_variant, p.alt_count, p.co_alt_count,
                                                                p.scoring_window)], host=True)
    assert_same_scores(fused, host)
    assert len(fused[0]) == sum(max(12 - s, 0) for s in pc.strides_of(4)) == 20 and stats[0]["launches"] == 1 and stats[0]["n_inf"] == 0


def test_a_batch_of_minus_infinity_entries_touches_no_device():
    p = synthetic(6, 9, seed=41, types=(gc.DN,), window=7)   # duplex variants only: the stored entries are the pairs within one variant
    stats: list = []
    got = progeny.score_variants_from_depths([p, p], device=12345, stats=stats)   # (no such device: nothing may ask for it)
    assert len(got[0]) == 6 and (got[0].scores_f64() == -np.inf).all() and all(s["launches"] == 0 and s["n_inf"] == 6 for s in stats)
