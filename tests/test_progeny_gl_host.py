"""CPU: the progeny genotype likelihoods on the host twin of the debug library (the kernel's cell function on one thread) against what the
reference's get_offspring_gl / compute_gt_likelihoods / correct_variant_types recorded (tests/golden/make_progeny_gl_golden.py), against
exact values computed here, the inputs the library refuses, and the Python mirrors on the recorded stand-in tables.

The bound B(n, k) = gamma(2n + k + 1) of the twin against the exact value is derived at progeny_gl_cases.bound; E_ref is the reference's
own largest deviation from the exact values, recorded by the generator."""
import numpy as np
import pytest

import progeny_gl_cases as gc
from whatshap_amd import _native, progeny

GOLD = gc.load_golden()
CASES = GOLD["cases"]
IDS = [c["spec"]["name"] for c in CASES]
E_REF = float.fromhex(GOLD["e_ref"])


def make(rec):
    """(case, problem, varinfo after from_tables) of a recorded case."""
    case = gc.Case(rec["spec"])
    assert case.sha256() == rec["inputs_sha256"], "the case generator no longer produces the recorded inputs"
    info = case.varinfo()
    return case, progeny.DepthProblem.from_tables(case.variant_table, case.progeny_table, case.offspring, info, case.param), info


def cell_depths(problem):
    """n = ref_dp + alt_dp of every table cell, [n_nodes][n_samples]."""
    n = problem.ref_depth.astype(np.int64) + problem.alt_depth
    return n[:, problem.node_row].T


def test_cases_cover_what_they_should():
    specs = [c["spec"] for c in CASES]
    assert {s["ploidy"] for s in specs} >= {2, 3, 4, 6, 8}
    assert any(not c["nodes"] for c in CASES) and sum(len(c["nodes"]) * c["spec"]["n_samples"] for c in CASES) > 1500
    assert 1e-15 < E_REF < 1e-11 and float.fromhex(GOLD["min_sum"]) > 1e-280
    shared = removed = 0
    for rec in CASES:
        case, problem, info = make(rec)
        shared += int((np.diff(problem.node_row) == 0).sum())
        removed += len(case.varinfo().get_phasable()) - len(info.get_phasable())
    assert shared > 20 and removed > 10


@pytest.mark.parametrize("rec", CASES, ids=IDS)
def test_host_table_equals_the_reference(rec):
    k1 = rec["spec"]["ploidy"] + 1
    case, problem, info = make(rec)
    assert gc.state_of(info) == rec["after_gl"] and info.get_node_positions() == rec["nodes"]
    f64: list = []
    table = progeny.offspring_gl_batch([problem], host=True, doubles=f64)[0]
    shape = (len(rec["nodes"]), len(case.offspring), k1)
    assert table.array().shape == shape
    assert np.array_equal(table.array().view(np.uint32), gc.unpack(rec["f32_bits"], "<u4").reshape(shape))
    want = gc.unpack(rec["f64"], "<f8").reshape(shape)
    m = 2.0 * cell_depths(problem) + k1
    tol = (m * 2.0 ** -53 / (1 - m * 2.0 ** -53) + E_REF)[:, :, None] * np.abs(want)
    assert np.array_equal(want < 0, f64[0] < 0) and (np.abs(f64[0] - want) <= tol).all()
    assert np.array_equal(f64[0].astype(np.float32).view(np.uint32), table.array().view(np.uint32))


# ---------------------------------------------------------------------------------------------- exact values
@pytest.mark.parametrize("ploidy", (2, 4, 6, 8))
@pytest.mark.parametrize("prior", list(gc.PRIOR_TYPES))
def test_host_against_exact_values(ploidy, prior):
    cells, problem = gc.exact_problem(ploidy, gc.PRIOR_TYPES[prior])
    if prior == "duplex_nulliplex":
        assert ploidy == 2 or 0.0 in problem.priors[2, 0]   # a prior row with zeros
    f64: list = []
    table = progeny.offspring_gl_batch([problem], host=True, doubles=f64)[0]
    gc.check_exact(cells, problem, f64[0], table.array())


def test_cells_the_reference_cannot_do_are_normalised_here():
    """The divergence: at these cells every pmf of the reference underflows -- the generator recorded a normalising sum of 0 and
    ZeroDivisionError or NaN --, here the values are finite, sum to 1 and put the weight on the nearest genotypes."""
    recorded = GOLD["underflowing"]
    assert [(r["ref_dp"], r["alt_dp"]) for r in recorded] == gc.UNDERFLOWING
    for r in recorded:
        assert float.fromhex(r["normalising_sum"]) == 0.0 and r["outcome"] in ("ZeroDivisionError", "nan")
        f64: list = []
        progeny.offspring_gl_batch([progeny.DepthProblem([[r["ref_dp"]]], [[r["alt_dp"]]], r["ploidy"], r["error_rate"])], host=True, doubles=f64)
        gl = f64[0][0, 0]
        exact = [float(x) for x in gc.decimal_cell(r["ref_dp"], r["alt_dp"], r["ploidy"], r["error_rate"])]
        assert np.isfinite(gl).all() and abs(gl.sum() - 1.0) <= 5 * 2.0 ** -53 and int(np.argmax(gl)) == int(np.argmax(exact))


# ---------------------------------------------------------------------------------------------- refused inputs
def test_invalid_inputs_are_refused_with_their_message():
    one = [[5]]

    def refused(match, *args, **kw):
        with pytest.raises(ValueError, match=match):
            progeny.offspring_gl_batch([progeny.DepthProblem(*args, **kw)], host=True)

    refused("ploidy 1 below 2", one, one, 1, 0.06)
    refused("ploidy 0 below 2", one, one, 0, 0.06)
    for rate in (0.0, 1.0, -0.1, 1.5, float("nan")):
        refused(r"error_rate .* outside \(0, 1\)", one, one, 4, rate)
    pri = progeny.compute_gt_likelihood_priors(4)
    refused(r"depth row 0 has \(alt_count, co_alt_count\) = \(5, 0\), above the ploidy 4", one, one, 4, 0.06, priors=pri, row_alt_count=[5], row_co_alt_count=[0])
    refused(r"depth row 0 has \(alt_count, co_alt_count\) = \(1, 7\), above the ploidy 4", one, one, 4, 0.06, priors=pri, row_alt_count=[1], row_co_alt_count=[7])
    refused("node 1 names depth row 1, but only 1 rows were given", one, one, 4, 0.06, node_row=[0, 1])
    bad = np.array(pri)
    bad[1, 0] = 0.0
    refused(r"priors\[1\]\[0\] \(depth row 0\) is negative, not finite or all zero", one, one, 4, 0.06, priors=bad, row_alt_count=[1], row_co_alt_count=[0])
    # the reference's uint32 index: (n_nodes + 1) * n_samples * (ploidy + 1) >= 2^32 (one depth row shared by all nodes keeps the input small)
    n_nodes = 2 ** 32 // (5 * 200)
    problem = progeny.DepthProblem(np.full((200, 1), 5), np.full((200, 1), 5), 4, 0.06, node_row=np.zeros(n_nodes, dtype=np.uint32))
    views = progeny._depth_views([problem])
    L = _native.debug_lib()
    assert L.whamd_debug_progeny_gl_host(views, 1, None, None) == _native.WHAMD_ERR_INVALID
    assert b"(n_nodes + 1) * n_samples * (ploidy + 1) reaches 2^32" in L.whamd_last_error()
    with pytest.raises(ValueError, match="outside 0 .. 2\\^32 - 1"):
        progeny.DepthProblem([[-1]], one, 4, 0.06)
    with pytest.raises(ValueError, match="mismatched lengths"):
        progeny.DepthProblem(one, [[1, 2]], 4, 0.06)


# ---------------------------------------------------------------------------------------------- the Python mirrors
@pytest.mark.parametrize("rec", CASES, ids=IDS)
def test_mirrors_on_the_recorded_tables(rec):
    k1 = rec["spec"]["ploidy"] + 1
    case = gc.Case(rec["spec"])
    # get_offspring_gl: the table, the removed variants
    info = case.varinfo()
    before = info.get_phasable()
    table = progeny.get_offspring_gl(case.variant_table, case.progeny_table, case.offspring, info, case.param, host=True)
    assert (table.getPloidy(), table.getNumSamples(), table.getNumPositions()) == (k1 - 1, len(case.offspring), len(rec["nodes"]))
    assert np.array_equal(table.array().view(np.uint32), gc.unpack(rec["f32_bits"], "<u4").reshape(table.array().shape))
    assert gc.state_of(info) == rec["after_gl"]
    removed = sorted(set(before) - set(info.get_phasable()))
    lookup = {}
    for i, v in enumerate(case.progeny_table.variants):
        if v.position:
            lookup[v.position] = i
    assert removed == [p for p in before if case.variant_table.variants[p].position not in lookup]
    # compute_gt_likelihoods: one sample, with and without priors; a node at the progeny position of the node before it repeats its list
    nodes = info.get_node_positions()
    pairs = [(v, lookup[case.variant_table.variants[v].position]) for v in nodes]
    want = gc.unpack(rec["f64"], "<f8").reshape(len(nodes), len(case.offspring), k1)
    plain = gc.unpack(rec["f64_no_priors_sample0"], "<f8").reshape(len(nodes), k1)
    tol = gc.bound(rec["spec"]["max_depth"], k1 - 1) + E_REF
    for priors, ref in ((progeny.compute_gt_likelihood_priors(k1 - 1), want[:, 0] if case.offspring else None), (None, plain)):
        if not case.offspring:
            continue
        got = progeny.compute_gt_likelihoods(case.progeny_table, case.offspring[0], pairs, info, case.param, priors, host=True)
        assert len(got) == len(nodes)
        for n, gl in enumerate(got):
            if ref[n, 0] < 0:
                assert gl is None
            else:
                assert len(gl) == k1 and all(abs(a - b) <= tol * b for a, b in zip(gl, ref[n].tolist()))
            if n and pairs[n][1] == pairs[n - 1][1]:
                assert gl is got[n - 1]
    # correct_variant_types: the state it leaves
    info = case.varinfo()
    progeny.correct_variant_types(case.variant_table, case.progeny_table, case.offspring, info, case.param, host=True)
    assert gc.state_of(info) == rec["after_correct"]


def test_nodes_of_one_progeny_position_share_the_first_nodes_row():
    """Two parent variants at one position with different alleles and types: the reference keys the reuse on the progeny position, so the
    second variant's nodes carry the first's likelihoods."""
    vt = gc.Table([500, 500, 900])
    pt = gc.Table([500, 900], {"a": [(30, 10, 4), (12, 12)], "b": [(2, 1, 0), (40, 1)]})
    info = gc.VariantInfo([gc.SN, gc.DN, gc.S2])
    info.append(0, 1, 1, 0)
    info.append(0, 2, 2, 0)
    info.append(1, 0, 1, 1)
    problem = progeny.DepthProblem.from_tables(vt, pt, ["a", "b"], info, gc.Param(4, 0.06))
    assert problem.node_row.tolist() == [0, 0, 0, 1] and problem.node_variant.tolist() == [0, 1, 1, 2]
    assert problem.ref_depth.tolist() == [[30, 12], [2, 1]] and problem.alt_depth.tolist() == [[10, 12], [1, 40]]
    assert (problem.row_alt_count.tolist(), problem.row_co_alt_count.tolist()) == ([1, 1], [0, 1])
    table = progeny.offspring_gl_batch([problem], host=True)[0].array()
    assert np.array_equal(table[0], table[1]) and np.array_equal(table[0], table[2]) and (table[0, 1] == -1).all() and table[0, 0, 0] > 0
