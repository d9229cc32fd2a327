"""The f64 range of the genotyper's run path (whatshap_amd/csrc/genotype_plan.h, GS_RESCALE / GS_MIN_TOTAL), on the host alone.

The long-double restatement (oracle/genotype_oracle.py) returns what its per-column normalisation divides out: the factor by which a chain
that is NOT rescaled shrinks in every column.  The debug library exports the run plan: which columns form a run and which runs rescale on
entry.  From the two, `exponent_model` works out how small the numbers of the device get, without a device:
  * every input of tests/test_gpu_genotype_range.py really is in the regime it is listed under (so that a later change of the generator cannot
    empty those tests), and is eligible for the run path;
  * under the exported schedule the stored chains and their product stay above 1e-290 on every table the run path keeps, and the model says
    which tables the device hands over to the per-column kernels (scaled column total below GS_MIN_TOTAL) -- genotype_cases.RUN_PATH, which the GPU
    tests hold the device to;
  * the compiled reference class is finite on these inputs and agrees with the restatement;
  * every rescaling run reads exactly the partial sums its neighbour emits."""
import functools

import numpy as np
import pytest

from genotype_cases import RANGE_CASES, RUN_PATH, range_case, reference_likelihoods
from oracle import genotype_oracle
from refobjects import reference_core
from whatshap_amd import _native

RESTATED = [name for name, (regime, _) in RANGE_CASES.items() if regime != "long"]
SMALLEST_NORMAL = -308.0   # log10 of the smallest normal f64, rounded towards zero (2.2e-308)
FLOOR = -290.0             # the model must stay above: the 53-bit mantissa clear of the subnormals, two decades for "sum instead of maximum"
@functools.lru_cache(maxsize=None)
def restated(name):
    """(problem, likelihoods of the restatement as float64, its normalisers) -- computed once per session."""
    problem = range_case(**RANGE_CASES[name][1])
    normalisers = {}
    gl = np.asarray(genotype_oracle.genotype_likelihoods(problem, normalisers=normalisers), dtype=np.float64)
    return problem, gl, normalisers


def worst_window(log_shrink, length):
    """The most negative sum of `length` consecutive entries (the whole array when it is shorter)."""
    length = min(int(length), log_shrink.size)
    total = np.concatenate(([0.0], np.cumsum(log_shrink)))
    return float((total[length:] - total[:-length]).min())


def transition_growth(problem):
    """log10 per column of what the device's transition adds to a chain's total: it applies P(j -> i) / P(i -> i) (one fused multiply-add
    per transmission bit with rho = r / (1 - r)), i.e. the reference's normalised transition times (1 - r)^(-2 triples)."""
    n_triples = problem.triple_ids.size // 3
    r = 10.0 ** (-np.asarray(problem.recombcost, dtype=np.float64) / 10.0)
    r[0] = 0.0   # (nothing transitions into the first column)
    return -2.0 * n_triples * np.log10(1.0 - r)


def exponent_model(runs, normalisers, growth):
    """Per column, log10 of what the device stores under the exported schedule: (forward, backward, forward * backward, column total).
    forward / backward: the TOTAL of the stored column (an upper bound of its largest entry, at most log10(cells) above it); the product of
    the two bounds every forward * backward the combine kernel forms; the column total is sum forward * backward * emission * prior, the number
    geno_slot_finish divides by and compares with GS_MIN_TOTAL -- exact, not a bound.
    A forward run stores column c BEFORE multiplying by its emission (after the transition into it), a backward run likewise (before the
    transition out of it); a rescaling run starts from a total of 1."""
    fwd, bwd, comb = normalisers["forward"], normalisers["backward"], normalisers["combined"]
    n = fwd.size
    f, b = np.zeros(n), np.zeros(n)
    level = 0.0
    for run in runs:
        if run["rescale_f"]:
            level = 0.0
        for c in range(run["c0"], run["c0"] + run["ncols"]):
            if c > 0:
                level += growth[c]
            f[c] = level
            level += fwd[c]
    level = 0.0
    for run in reversed(runs):
        if run["rescale_b"]:
            level = 0.0
        for c in range(run["c0"] + run["ncols"] - 1, run["c0"] - 1, -1):
            b[c] = level
            if c > 0:
                level += growth[c] + bwd[c - 1]
    return f, b, f + b, f + b + comb


@pytest.mark.parametrize("name", list(RANGE_CASES))
def test_every_case_is_eligible_for_the_run_path(name):
    problem = range_case(**RANGE_CASES[name][1])
    plan = _native.plan_summary(problem, "genotype_slots")
    assert plan["invariants_ok"] == 1 and plan["n_resident_columns"] == plan["n_columns"] == problem.n_variants, plan
    assert _native.debug_genotype_run_plan(problem) is not None


@pytest.mark.parametrize("name", RESTATED)
def test_every_case_is_in_its_regime(name):
    """By the restatement's forward normalisers alone (the backward ones tell the same: asserted too)."""
    regime = RANGE_CASES[name][0]
    problem, _, normalisers = restated(name)
    longest = _native.plan_summary(problem, "genotype_slots")["max_run_columns"]
    shrink = normalisers["forward"]
    mean, one, four, seven = float(shrink.mean()), worst_window(shrink, longest), worst_window(shrink, 4 * longest), worst_window(shrink, 7 * longest)
    print(f"{name}: longest run {longest} columns; log10 shrink: mean {mean:.2f} per column, worst run {one:.0f}, worst 4 runs {four:.0f}, worst 7 runs {seven:.0f}")
    assert abs(float(normalisers["backward"].mean()) - mean) < 0.25
    assert longest >= 20   # (32 at these coverages today; the thresholds below are per run, whatever its length)
    if regime == "deep":
        assert one < -150 and mean < -150 / longest
    elif regime == "chain":
        assert four < SMALLEST_NORMAL and one > -150 and mean < -2.0
    elif regime == "product":
        assert four > SMALLEST_NORMAL and seven < SMALLEST_NORMAL and -2.5 < mean < -1.5
    elif regime == "inside":
        assert seven > FLOOR and seven < -150 and -1.5 < mean < -0.7   # more than half of the exponent range in use
    elif name.startswith("confident"):
        uniform = float(restated(name.replace("confident", "uniform"))[2]["forward"].mean())
        assert mean < uniform - 3.0 and one < -150   # the priors, not the reads, make the shrink: the deep regime by another route
    else:
        assert -1.5 < mean < -0.5 and seven > FLOOR


@pytest.mark.parametrize("name", RESTATED)
def test_reference_class_is_finite_and_agrees_with_the_restatement(name):
    ref = reference_core()
    problem, gl, _ = restated(name)
    want = reference_likelihoods(problem, ref)
    assert np.isfinite(want).all() and np.isfinite(gl).all()
    assert np.allclose(gl, want, rtol=1e-9, atol=1e-13), np.abs(gl - want).max()
    assert np.allclose(want.sum(axis=2), 1.0, rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", RESTATED)
def test_exponent_model_stays_in_range_or_the_table_leaves_the_run_path(name):
    problem, _, normalisers = restated(name)
    runs, min_total = _native.debug_genotype_run_plan(problem)
    assert sum(run["ncols"] for run in runs) == problem.n_variants and runs[0]["c0"] == 0
    f, b, product, total = exponent_model(runs, normalisers, transition_growth(problem))
    lowest = float(total.min())
    print(f"{name}: {len(runs)} runs; log10 minima: forward {f.min():.0f}, backward {b.min():.0f}, product {product.min():.0f}, column total {lowest:.0f}"
          f" (column {int(total.argmin())}); hand-over below {np.log10(min_total):.0f}")
    assert 1e-200 < min_total < 1e-100
    # the prediction does not hang on the last digits: no case within two decades of the hand-over
    assert abs(lowest - np.log10(min_total)) > 2.0
    keeps = lowest > np.log10(min_total)
    assert keeps == RUN_PATH[name]
    if keeps:
        assert f.min() > FLOOR and b.min() > FLOOR and product.min() > FLOOR
        assert max(f.max(), b.max()) < 200.0   # (a pedigree's transition GROWS the totals: far from 1e308 as well)
    else:
        # what the hand-over is for: by the model the run path's own numbers would not all be trustworthy here, or nearly so
        assert product.min() < np.log10(min_total)


def _problem_with_runs(n_runs):
    """A table of the synthetic generator that the planner cuts into exactly n_runs runs."""
    for n_variants in range(4, 400):
        problem = range_case(n_variants, 6, 2, 0.02, None, seed=1)
        planned = _native.debug_genotype_run_plan(problem)
        if planned is not None and len(planned[0]) == n_runs:
            return planned[0]
    raise AssertionError(f"no table with {n_runs} runs")


@pytest.mark.parametrize("n_runs", [1, 2, 4, 5, 9])
def test_rescaling_runs_read_what_their_neighbours_emit(n_runs):
    runs = _problem_with_runs(n_runs)
    spans = []
    for ri, run in enumerate(runs):
        assert run["c0"] == (runs[ri - 1]["c0"] + runs[ri - 1]["ncols"] if ri else 0)
        for direction, neighbour in (("f", ri - 1), ("b", ri + 1)):
            spans.append((run[f"part_out_{direction}"], run["n_part_out"]))
            if not 0 <= neighbour < n_runs:   # nothing enters the chain's first run: nothing to rescale by, and nobody reads behind its last
                assert run[f"rescale_{direction}"] == 0 and run[f"n_part_in_{direction}"] == 0
                assert run["emit_b" if direction == "f" else "emit_f"] == 0
                continue
            other = runs[neighbour]
            assert run[f"rescale_{direction}"] == other[f"emit_{direction}"]   # emitted exactly when read
            if run[f"rescale_{direction}"]:
                assert (run[f"part_in_{direction}"], run[f"n_part_in_{direction}"]) == (other[f"part_out_{direction}"], other["n_part_out"])
            else:
                assert run[f"n_part_in_{direction}"] == 0
    spans.sort()
    assert all(a + n <= b for (a, n), (b, _) in zip(spans, spans[1:]))   # no two runs write the same sums
    # both chains rescale at the same boundaries (the product of the two never carries more than one group of runs), and no chain goes
    # further than a group without rescaling
    for ri in range(1, n_runs):
        assert runs[ri]["rescale_f"] == runs[ri - 1]["rescale_b"]
    assert all(run["rescale_f"] for run in runs[1:]) and all(run["rescale_b"] for run in runs[:-1])   # every run: GS_RESCALE = 1
