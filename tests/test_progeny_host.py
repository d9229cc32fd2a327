"""CPU: progeny marker scoring on the host twin of the debug library (the device's inner function on one thread) against what the compiled
reference and the reference's own Python loop recorded (tests/golden/make_progeny_golden.py): the stored entries, their double scores bit
for bit, their float bits; the mirror class's getters and single-pair scores with the reference's quirks; compute_gt_likelihood_priors
and the variant types; the inputs the library refuses."""
import math

import numpy as np
import pytest

import progeny_cases as pc
from whatshap_amd import progeny

GOLD = pc.load_golden()
PAIR_CASES = GOLD["pair_cases"]
IDS = [c["spec"]["name"] for c in PAIR_CASES]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def make_table(rec):
    """The mirror class filled as the generator filled the reference's, and the inputs."""
    spec = rec["spec"]
    table, node_variant, alt, co = pc.build_pair_case(spec)
    assert pc.table_sha256(table) == rec["table_sha256"], "the case generator no longer produces the recorded inputs"
    t = progeny.ProgenyGenotypeLikelihoods(spec["ploidy"], spec["n_samples"], rec["n_positions"])
    for pos in range(table.shape[0]):
        for s in range(table.shape[1]):
            if table[pos, s, 0] >= 0:
                t.setGlv(pos, s, [float(x) for x in table[pos, s]])
    for b in rec["set_beyond"]:
        t.setGlv(b["pos"], b["sample"], [float.fromhex(x) for x in b["row"]])
        t.setGl(b["pos"], b["sample"], 0, 0.25)
    assert np.array_equal(t.array().view(np.uint32), table.view(np.uint32))
    return t, node_variant, alt, co


def test_cases_cover_what_they_should():
    specs = [c["spec"] for c in PAIR_CASES]
    assert {s["ploidy"] for s in specs} >= {2, 3, 4, 6, 8}
    assert {s["window"] for s in specs} >= {1, 2, 4, 7, 50, 250}
    assert min(s["n_samples"] for s in specs) <= 1 and max(s["n_samples"] for s in specs) == 300
    assert sum(c.get("n_entries", 0) for c in PAIR_CASES) > 400_000


@pytest.mark.parametrize("rec", PAIR_CASES, ids=IDS)
def test_host_scores_equal_the_reference_bit_for_bit(rec):
    spec = rec["spec"]
    t, node_variant, alt, co = make_table(rec)
    varinfo, param = pc.VarInfo(node_variant, alt, co), pc.Param(spec["window"])
    if "raises" in rec:
        assert rec["raises"] == "IndexError" and spec["window"] < 4   # the reference's stride list fails there
        with pytest.raises(ValueError, match="stride list is undefined"):
            progeny.get_variant_scoring(varinfo, t, param, host=True)
        return
    st = {}
    got = progeny.get_variant_scoring(varinfo, t, param, host=True, stats=st)
    i, j, f32 = got.arrays()
    f64 = got.scores_f64()
    assert len(got) == rec["n_entries"] == st["n_entries"]
    # the complete list against the recorded digest, the recorded entries one by one
    assert pc.entries_digest(i, j, f64, f32.view(np.uint32)) == rec["digest"]
    step = rec["step"]
    assert np.array_equal(i[::step], pc.unpack(rec["i"], "<u4")) and np.array_equal(j[::step], pc.unpack(rec["j"], "<u4"))
    assert np.array_equal(bits(f64[::step]), pc.unpack(rec["f64"], "<f8").view(np.uint64))
    assert np.array_equal(f32[::step].view(np.uint32), pc.unpack(rec["f32_bits"], "<u4"))
    # what the inputs alone say: the entry set, the -inf and reused counts, the restated scores
    hi, lo, eff, kind, reused = pc.derive_entries(node_variant, alt, co, spec["window"])
    assert np.array_equal(i, hi) and np.array_equal(j, lo)
    assert st["n_inf"] == int((kind == pc.KIND_INF).sum()) == int(np.isneginf(f64).sum())
    assert st["n_reused"] == int(reused.sum())
    assert st["n_sample_terms"] == (len(got) - st["n_inf"]) * spec["n_samples"]
    assert st["launches"] == 0
    if len(got) <= 50_000:
        restated, n, big = pc.restate_scores(t.array(), len(node_variant), spec["ploidy"], lo, eff, kind)
        assert np.all(np.isneginf(restated) == np.isneginf(f64))
        fin = ~np.isneginf(f64)
        assert np.all(np.abs(restated[fin] - f64[fin]) <= pc.bound(n[fin], big[fin]))   # (numpy's log against the C library's)
    # the float scores are the doubles rounded
    with np.errstate(over="ignore"):
        assert np.array_equal(f64.astype(np.float32).view(np.uint32), f32.view(np.uint32))


def test_reused_scores_are_the_earlier_nodes():
    """duplex_runs gives the two nodes of a duplex variant different rows: the second node's entry must repeat the first's score."""
    rec = next(c for c in PAIR_CASES if c["spec"]["name"] == "duplex_runs")
    t, node_variant, alt, co = make_table(rec)
    got = progeny.get_variant_scoring(pc.VarInfo(node_variant, alt, co), t, pc.Param(rec["spec"]["window"]), host=True)
    i, j, _ = got.arrays()
    hi, lo, eff, kind, reused = pc.derive_entries(node_variant, alt, co, rec["spec"]["window"])
    assert reused.sum() >= 5
    score = {(int(a), int(b)): s for a, b, s in zip(i, j, got.scores_f64())}
    for h, l, e in zip(hi[reused], lo[reused], eff[reused]):
        assert e != h and score[(int(h), int(l))] == score[(int(e), int(l))]
        assert t.getDuplexNulliplexScore(int(l), int(h)) != score[(int(h), int(l))]   # its own row would have given another score


@pytest.mark.parametrize("rec", PAIR_CASES, ids=IDS)
def test_mirror_class_getters(rec):
    spec = rec["spec"]
    t, node_variant, _, _ = make_table(rec)
    assert t.getNumPositions() == len(t) == rec["num_positions_after"] == rec["n_positions"]   # rows set beyond it do not raise it
    assert t.getPloidy() == spec["ploidy"] and t.getNumSamples() == spec["n_samples"]
    for g in rec["getters"]:
        assert float(t.getGl(g["pos"], g["sample"], g["genotype"])).hex() == g["gl"]
        assert [float(x).hex() for x in t.getGlv(g["pos"], g["sample"])] == g["glv"]
    for b in rec["set_beyond"]:
        assert t.getGl(b["pos"], b["sample"], 0) == 0.0 and t.getGlv(b["pos"], b["sample"]) == [0.0] * (spec["ploidy"] + 1)
    for p in rec["pair_scores"]:
        assert float(t.getSimplexNulliplexScore(p["pos1"], p["pos2"])).hex() == p["sn"]
        assert float(t.getSimplexSimplexScore(p["pos1"], p["pos2"])).hex() == p["s2"]
        assert float(t.getDuplexNulliplexScore(p["pos1"], p["pos2"])).hex() == p["dn"]


def test_values_are_kept_as_floats():
    t = progeny.ProgenyGenotypeLikelihoods(4, 2, 3)
    assert t.getGl(1, 1, 2) == -1.0
    t.setGl(1, 1, 2, 0.1)
    assert t.getGl(1, 1, 2) == float(np.float32(0.1)) != 0.1
    a = np.arange(30, dtype=np.float64).reshape(3, 2, 5) / 7
    u = progeny.ProgenyGenotypeLikelihoods.from_array(a)
    assert (u.getPloidy(), u.getNumSamples(), u.getNumPositions()) == (4, 2, 3)
    assert u.getGlv(2, 1) == [float(x) for x in a[2, 1].astype(np.float32)]


def test_entries_of_a_given_list():
    rec = next(c for c in PAIR_CASES if c["spec"]["name"] == "mixed_p4_w50")
    t, node_variant, alt, co = make_table(rec)
    problem = progeny.ProgenyProblem(t, node_variant, alt, co, rec["spec"]["window"])
    full = progeny.score_variants_batch([problem], host=True)[0]
    i, j, _ = full.arrays()
    stored, score = progeny.score_entries_host(problem, j, i)          # either order
    assert stored.all() and np.array_equal(bits(score), bits(full.scores_f64()))
    have = set(zip(i.tolist(), j.tolist()))
    n = len(node_variant)
    others = [(a, b) for a in range(n) for b in range(a) if (a, b) not in have] + [(n + 3, 0), (2, 2)]
    stored, _ = progeny.score_entries_host(problem, [a for a, _ in others], [b for _, b in others])
    assert not stored.any()


def test_priors_equal_the_reference_bit_for_bit():
    assert sorted(int(k) for k in GOLD["priors"]) == list(range(2, 13))
    for k, recorded in GOLD["priors"].items():
        got = progeny.compute_gt_likelihood_priors(int(k))
        assert [[[float(x).hex() for x in d] for d in row] for row in got] == recorded
        assert got[1][0] is got[0][1]


@pytest.mark.parametrize("rec", GOLD["type_cases"], ids=[c["spec"]["name"] for c in GOLD["type_cases"]])
def test_variant_types_on_the_host(rec):
    spec = rec["spec"]
    priors = progeny.compute_gt_likelihood_priors(spec["ploidy"])
    table, truth = pc.build_type_case(spec, priors)
    assert pc.table_sha256(table) == rec["table_sha256"] and [list(t) for t in truth] == rec["truth"]
    t = progeny.ProgenyGenotypeLikelihoods.from_array(table)
    winners, llh = progeny.most_likely_variant_types(priors, t, host=True)
    expected = pc.unpack(rec["llh"], "<f8").reshape(llh.shape)
    assert np.array_equal(bits(llh), bits(expected))      # the same C library's log as Python's
    assert [list(w) for w in winners] == rec["winners"]
    # a subset of the rows, a row beyond the table (all zeros: every type is -inf, the winner stays (0, 0))
    nodes = [3, 0, table.shape[0] + 2]
    w2, l2 = progeny.most_likely_variant_types(priors, t, nodes=nodes, host=True)
    assert w2[:2] == [winners[3], winners[0]] and np.array_equal(bits(l2[:2]), bits(llh[[3, 0]]))
    assert w2[2] == (0, 0) and np.all(np.isneginf(l2[2]))


def test_python_log_is_the_librarys_log():
    """The recorded llh values came from Python's math.log; the host twin uses the C library's.  They are the same function here -- if this
    ever fails, the bit-for-bit comparison above is reporting a platform difference, not a defect."""
    rec = GOLD["type_cases"][2]
    priors = progeny.compute_gt_likelihood_priors(rec["spec"]["ploidy"])
    table, _ = pc.build_type_case(rec["spec"], priors)
    t = progeny.ProgenyGenotypeLikelihoods.from_array(table)
    _, llh = progeny.most_likely_variant_types(priors, t, nodes=[0], host=True)
    k1 = rec["spec"]["ploidy"] + 1
    types = [(g0, g1) for g0 in range(k1) for g1 in range(g0 + 1)]
    for ty, (g0, g1) in enumerate(types):
        total = 1.0
        for s in range(t.getNumSamples()):
            if t.getGl(0, s, 0) < 0.0:
                continue
            like = 0.0
            for g in range(k1):
                like += priors[g0][g1][g] * t.getGl(0, s, g)
            total = total - math.inf if like <= 0.0 else total + math.log(like)
        assert total == llh[0, ty] or (math.isinf(total) and math.isinf(llh[0, ty]))


def small_problem(**kw):
    types = kw.pop("types", [pc.SN] * 6)
    ploidy = kw.pop("ploidy", 4)
    window = kw.pop("window", 7)
    n_samples = kw.pop("n_samples", 3)
    n_nodes = sum(t[0] for t in types)
    t = progeny.ProgenyGenotypeLikelihoods(ploidy, n_samples, n_nodes)
    node_variant = [v for v, ty in enumerate(types) for _ in range(ty[0])]
    return progeny.ProgenyProblem(t, node_variant, [ty[0] for ty in types], [ty[1] for ty in types], window)


@pytest.mark.parametrize("host", [True, False])
def test_invalid_inputs_raise_with_the_librarys_message(host):
    """Validation comes before any device work, in both libraries."""
    def run(p):
        return progeny.score_variants_batch([p], host=host)

    with pytest.raises(ValueError, match="ploidy 1 below 2"):
        run(small_problem(ploidy=1))
    with pytest.raises(ValueError, match="scoring_window must be at least 1"):
        run(small_problem(window=0))
    with pytest.raises(ValueError, match="scoring_window 3 below 4"):
        run(small_problem(window=3))
    p = small_problem()
    p.node_variant[2] = 17
    with pytest.raises(ValueError, match="node 2 names variant 17.*mismatched lengths"):
        run(p)
    with pytest.raises(ValueError, match="mismatched lengths"):
        progeny.ProgenyProblem(p.off_gl, [0, 1], [1, 1], [0], 7)
    # a triplex variant behind a simplex-nulliplex anchor has no score kind (the reference would store a stale value)
    with pytest.raises(ValueError, match=r"pair \(0, 1\): variant 1 has \(alt_count, co_alt_count\) = \(3, 0\), which has no score kind"):
        run(small_problem(types=[pc.SN, (3, 0), pc.SN]))
    with pytest.raises(ValueError, match="reaches 2\\^32"):
        progeny.ProgenyGenotypeLikelihoods(4, 1 << 16, 1 << 14)
    with pytest.raises(ValueError, match="mismatched lengths"):
        progeny.most_likely_variant_types(progeny.compute_gt_likelihood_priors(3), p.off_gl, host=True)
