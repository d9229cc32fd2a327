"""GPU: progeny marker scoring on the device.  Against every recorded result of the reference (tests/golden/make_progeny_golden.py), one
by one and as one batch, within the bound derived below; the variant types; a chromosome-sized problem (60 000 nodes x 200 samples,
window 250) against the entry set derived in numpy and the debug library's host twin; determinism; a batch of 200 problems against the
same problems one by one; and the calls that need no device work.

The bound.  Products, sums and the division are rounded one by one on host and device alike (no contraction), so the arguments of log are
the reference's bit for bit.  The device's log is specified to 3 ulp, the host's is below 1 ulp: 8 * 2^-53 relative per term.  The two
recursive sums of n + 1 terms add 2n * 2^-53 * S.  Hence |device - reference| <= 2^-53 (2n + 8) S with n the samples that contribute to
the entry and S = |log(1/(k-1))| + sum |log(cooccur / disjoint)| -- both computed by progeny_cases.restate_scores from the inputs, not by
the library.  -inf and NaN must be exactly that; the float score is the rounding of the device's double, within 1 float ulp of the
recorded one."""
import numpy as np
import pytest

import progeny_cases as pc
from whatshap_amd import progeny

pytestmark = pytest.mark.gpu

GOLD = pc.load_golden()
PAIR_CASES = [c for c in GOLD["pair_cases"] if "raises" not in c]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def f32_ulp_distance(a, b):
    def key(x):
        u = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(u < 0, -(u & 0x7FFFFFFF), u)
    return np.abs(key(a) - key(b))


def problem_of(rec):
    spec = rec["spec"]
    table, node_variant, alt, co = pc.build_pair_case(spec)
    assert pc.table_sha256(table) == rec["table_sha256"]
    return progeny.ProgenyProblem(progeny.ProgenyGenotypeLikelihoods.from_array(table), node_variant, alt, co, spec["window"])


def check_against_reference(rec, problem, got, host):
    """`got` from the device, `host` from the debug library's twin (bit-identical to the reference: tests/test_progeny_host.py)."""
    spec = rec["spec"]
    i, j, f32 = got.arrays()
    f64 = got.scores_f64()
    hi, lo, eff, kind, _ = pc.derive_entries(problem.node_variant, problem.alt_count, problem.co_alt_count, spec["window"])
    assert len(got) == rec["n_entries"] and np.array_equal(i, hi) and np.array_equal(j, lo)
    _, n, big = pc.restate_scores(problem.off_gl.array(), len(problem.node_variant), spec["ploidy"], lo, eff, kind)
    limit = pc.bound(n, big)
    ref = host.scores_f64()
    special = ~np.isfinite(ref)
    assert np.array_equal(bits(f64[special]), bits(ref[special]))            # -inf (and NaN) exactly
    err = np.abs(f64[~special] - ref[~special])
    print(f"{spec['name']}: {len(got)} entries, max |device - reference| = {err.max(initial=0.0):.3e}, smallest bound = "
          f"{limit[~special].min(initial=np.inf):.3e}, identical: {int((bits(f64) == bits(ref)).sum())}")
    assert np.all(err <= limit[~special])
    with np.errstate(over="ignore"):
        assert np.array_equal(f64.astype(np.float32).view(np.uint32), f32.view(np.uint32))
    # the recorded entries themselves
    step = rec["step"]
    assert np.array_equal(i[::step], pc.unpack(rec["i"], "<u4")) and np.array_equal(j[::step], pc.unpack(rec["j"], "<u4"))
    rec64 = pc.unpack(rec["f64"], "<f8")
    assert np.array_equal(bits(rec64), bits(ref[::step]))
    rec32 = pc.unpack(rec["f32_bits"], "<u4").view(np.float32)
    fin = np.isfinite(rec32)
    assert np.array_equal(f32[::step][~fin].view(np.uint32), rec32[~fin].view(np.uint32))
    assert f32_ulp_distance(f32[::step][fin], rec32[fin]).max(initial=0) <= 1


def test_device_equals_reference_case_by_case():
    launched = 0
    for rec in PAIR_CASES:
        problem = problem_of(rec)
        stats = []
        got = progeny.score_variants_batch([problem], stats=stats)[0]
        st = stats[0]
        host = progeny.score_variants_batch([problem], host=True)[0]
        check_against_reference(rec, problem, got, host)
        assert st["launches"] == (1 if st["n_entries"] > st["n_inf"] else 0)
        launched += st["launches"]
    assert launched >= 25


def test_device_equals_reference_as_one_batch():
    problems = [problem_of(rec) for rec in PAIR_CASES]
    stats = []
    got = progeny.score_variants_batch(problems, stats=stats)
    hosts = progeny.score_variants_batch(problems, host=True)
    assert all(st["launches"] == 1 for st in stats)       # one launch for all of them
    for rec, problem, g, h in zip(PAIR_CASES, problems, got, hosts):
        check_against_reference(rec, problem, g, h)


@pytest.mark.parametrize("rec", GOLD["type_cases"], ids=[c["spec"]["name"] for c in GOLD["type_cases"]])
def test_variant_types(rec):
    spec = rec["spec"]
    priors = progeny.compute_gt_likelihood_priors(spec["ploidy"])
    table, _ = pc.build_type_case(spec, priors)
    assert pc.table_sha256(table) == rec["table_sha256"]
    t = progeny.ProgenyGenotypeLikelihoods.from_array(table)
    winners, llh = progeny.most_likely_variant_types(priors, t)
    ref = pc.unpack(rec["llh"], "<f8").reshape(llh.shape)
    _, n, big = pc.restate_type_llh(table, priors)
    special = ~np.isfinite(ref)
    assert np.array_equal(bits(llh[special]), bits(ref[special]))
    err = np.abs(llh[~special] - ref[~special])
    print(f"{spec['name']}: max |device - reference| = {err.max(initial=0.0):.3e}, smallest bound = {pc.bound(n, big)[~special].min():.3e}")
    assert np.all(err <= pc.bound(n, big)[~special])
    assert [list(w) for w in winners] == rec["winners"]
    w2, l2 = progeny.most_likely_variant_types(priors, t, nodes=[2, table.shape[0] + 1])
    assert w2 == [winners[2], (0, 0)] and np.array_equal(bits(l2[0]), bits(llh[2])) and np.all(np.isneginf(l2[1]))


@pytest.fixture(scope="module")
def large():
    table, node_variant, alt, co, window = pc.large_problem()
    problem = progeny.ProgenyProblem(progeny.ProgenyGenotypeLikelihoods.from_array(table), node_variant, alt, co, window)
    stats = []
    got = progeny.score_variants_batch([problem], stats=stats)[0]
    derived = pc.derive_entries(problem.node_variant, problem.alt_count, problem.co_alt_count, problem.scoring_window)
    return problem, got, stats[0], derived


def test_large_problem_entry_set_and_counts(large):
    problem, got, st, (hi, lo, eff, kind, reused) = large
    assert st["n_nodes"] == 60_000 and st["n_entries"] >= 12_000_000 and st["launches"] == 1
    i, j, f32 = got.arrays()
    assert np.array_equal(i, hi) and np.array_equal(j, lo)
    assert st["n_inf"] == int((kind == pc.KIND_INF).sum()) > 0 and st["n_reused"] == int(reused.sum()) > 0
    assert st["n_sample_terms"] == (st["n_entries"] - st["n_inf"]) * 200
    f64 = got.scores_f64()
    assert np.array_equal(np.isneginf(f64), kind == pc.KIND_INF) and not np.isnan(f64).any()
    with np.errstate(over="ignore"):
        assert np.array_equal(f64.astype(np.float32).view(np.uint32), f32.view(np.uint32))
    print({k: (round(v, 2) if isinstance(v, float) else v) for k, v in st.items()})


def test_large_problem_sample_against_the_host_twin(large):
    problem, got, _, (hi, lo, eff, kind, _) = large
    pick = np.sort(np.random.default_rng(11).choice(hi.size, 20_000, replace=False))
    stored, ref = progeny.score_entries_host(problem, lo[pick], hi[pick])
    assert stored.all()
    _, n, big = pc.restate_scores(problem.off_gl.array(), len(problem.node_variant), 4, lo[pick], eff[pick], kind[pick])
    f64 = got.scores_f64()[pick]
    special = ~np.isfinite(ref)
    assert np.array_equal(bits(f64[special]), bits(ref[special]))
    err = np.abs(f64[~special] - ref[~special])
    limit = pc.bound(n, big)[~special]
    print(f"large: max |device - host twin| = {err.max():.3e}, smallest bound = {limit.min():.3e}, median n = {int(np.median(n))}, "
          f"identical: {int((bits(f64) == bits(ref)).sum())} of {pick.size}")
    assert np.all(err <= limit)


def test_two_device_runs_are_bit_identical(large):
    problem, got, _, _ = large
    again = progeny.score_variants_batch([problem])[0]
    assert all(np.array_equal(a, b) for a, b in zip(got.arrays()[:2], again.arrays()[:2]))
    assert np.array_equal(bits(got.scores_f64()), bits(again.scores_f64()))


def test_batch_of_200_problems_equals_one_by_one():
    problems = []
    for b in range(200):
        table, node_variant, alt, co, window = pc.large_problem(n_nodes=40 + 7 * (b % 23), n_samples=1 + b % 37, ploidy=(2, 3, 4, 6, 8)[b % 5],
                                                                window=(4, 7, 50, 250)[b % 4], seed=300 + b, p_dn=0.1, p_s2=0.1)
        problems.append(progeny.ProgenyProblem(progeny.ProgenyGenotypeLikelihoods.from_array(table), node_variant, alt, co, window))
    problems[7] = progeny.ProgenyProblem(progeny.ProgenyGenotypeLikelihoods(4, 3, 0), [], [], [], 250)   # an empty problem inside the batch
    stats = []
    batch = progeny.score_variants_batch(problems, stats=stats)
    assert len(batch) == 200 and all(st["launches"] == 1 for st in stats)       # one launch for all of them
    for p, b, st in zip(problems, batch, stats):
        one_stats = []
        one = progeny.score_variants_batch([p], stats=one_stats)[0]
        assert all(np.array_equal(x, y) for x, y in zip(b.arrays(), one.arrays()))
        assert np.array_equal(bits(b.scores_f64()), bits(one.scores_f64()))
        assert st["n_entries"] == one_stats[0]["n_entries"] and st["n_reused"] == one_stats[0]["n_reused"]


def test_no_launch_where_nothing_is_computed():
    empty = progeny.ProgenyProblem(progeny.ProgenyGenotypeLikelihoods(4, 5, 0), [], [], [], 250)
    one = progeny.ProgenyProblem(progeny.ProgenyGenotypeLikelihoods(4, 5, 1), [0], [1], [0], 250)
    types = [(3, 0), (2, 1), (4, 0), (2, 0)]
    nodes = [v for v, t in enumerate(types) for _ in range(t[0])]
    multiplex = progeny.ProgenyProblem(progeny.ProgenyGenotypeLikelihoods(6, 5, len(nodes)), nodes, [t[0] for t in types], [t[1] for t in types], 50)
    for problem, n_entries in ((empty, 0), (one, 0), (multiplex, 3 + 1 + 6 + 1)):
        stats = []
        got = progeny.score_variants_batch([problem], stats=stats)[0]
        assert len(got) == n_entries == stats[0]["n_inf"]
        assert np.all(np.isneginf(got.scores_f64())) and np.all(np.isneginf(got.arrays()[2]))
        assert stats[0]["launches"] == 0 and stats[0]["kernel_ms"] == 0.0
    stats = []
    assert progeny.score_variants_batch([empty, one, multiplex], stats=stats)[2].size() == 11 and all(st["launches"] == 0 for st in stats)
    assert progeny.score_variants_batch([]) == []
