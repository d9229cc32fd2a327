"""GPU (-m gpu): the genotyper where its f64 chains shrink fastest -- low coverage (runs of 32 columns), high qualities, reads in conflict,
confident priors against the reads, long tables -- against the compiled reference class (long double, rescaled every column).  The inputs
and what makes each of them hard are genotype_cases.RANGE_CASES; tests/test_genotype_range_host.py holds every input to its regime, the
reference class to the restatement, and predicts from the reference alone which tables the run path keeps (genotype_cases.RUN_PATH):
the others it must hand to the per-column kernels, which are held to the same tolerance here under a forced window."""
import functools

import numpy as np
import pytest

from genotype_cases import RANGE_CASES, RUN_PATH, range_case, reference_likelihoods
from refobjects import reference_core
from whatshap_amd import _native

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-9, 1e-13
WINDOWS = [0, 7]   # 0: the product's choice (the run path where it applies); a forced window: the per-column kernels


@functools.lru_cache(maxsize=None)
def case(name):
    """(problem, likelihoods of the reference class): once per session."""
    problem = range_case(**RANGE_CASES[name][1])
    return problem, reference_likelihoods(problem, reference_core())


def device_likelihoods(problem, window=0):
    return _native.genotype_likelihoods(problem, int(problem.n_variants), window=window)


def check(name, window):
    problem, want = case(name)
    got, stats = device_likelihoods(problem, window)
    finite = bool(np.isfinite(got).all())
    row_error = float(np.abs(got.sum(axis=2) - 1.0).max()) if finite else float("nan")
    worst = float(np.abs(got - want).max()) if finite else float("nan")
    print(f"{name} window {window}: slot_runs {stats['slot_runs']}, launches {stats['launches']}, finite {finite}, rows sum to 1 within {row_error:.2e}, "
          f"largest difference from the reference {worst:.2e}")
    assert finite, (name, window, int(np.isnan(got).any(axis=(0, 2)).sum()), "columns with NaN")
    assert row_error <= 1e-12
    assert np.allclose(got, want, rtol=RTOL, atol=ATOL), (name, window, worst, np.flatnonzero(~np.isclose(got, want, rtol=RTOL, atol=ATOL).all(axis=(0, 2)))[:10])
    # which path produced it: under a forced window the per-column kernels, else the run path exactly where the model says its range suffices
    assert (stats["slot_runs"] > 0) == (window == 0 and RUN_PATH[name]), (name, window, stats)
    return got, stats


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("name", ["deep_coverage6", "deep_coverage8"])
def test_one_run_alone_shrinks_by_more_than_150_decades(name, window):
    """Rescaling every run is not enough here: the table leaves the run path."""
    check(name, window)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("name", ["chain_single", "chain_trio"])
def test_a_chain_of_four_runs_would_underflow(name, window):
    check(name, window)


@pytest.mark.parametrize("window", WINDOWS)
def test_only_the_product_of_the_two_chains_would_underflow(window):
    check("product_step3", window)


@pytest.mark.parametrize("window", WINDOWS)
def test_hifi_qualities_phred93_at_two_percent_errors(window):
    """The realistic one: coverage 6, every quality 93, 2 % errors -- each chain stays normal over four runs, their product does not."""
    check("hifi_phred93", window)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("name", ["inside_generator", "inside_quartet"])
def test_close_to_the_limit_but_inside_stays_on_the_run_path(name, window):
    _, stats = check(name, window)
    assert (stats["slot_runs"] > 0) == (window == 0)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("name", ["confident_single", "confident_trio", "uniform_single", "uniform_trio"])
def test_confident_priors_against_the_reads_and_uniform_ones(name, window):
    check(name, window)


@pytest.mark.parametrize("name,window_bytes", [("long_single", 400_000), ("long_trio", 300_000)])
def test_long_tables_and_their_windowed_solve(name, window_bytes, monkeypatch):
    """Thousands of columns: no drift at the far end, and the windowed solve -- forward columns recomputed from the kept exchange column,
    rescaling included -- gives the SAME doubles."""
    problem, want = case(name)
    tail = slice(-50, None)
    for window in WINDOWS:
        got, stats = check(name, window)
        assert np.allclose(got[:, tail], want[:, tail], rtol=RTOL, atol=ATOL)
        if window == 0:
            whole, whole_stats = got, stats
    assert whole_stats["window"] == problem.n_variants
    monkeypatch.setenv("WHAMD_GENO_WINDOW_BYTES", str(window_bytes))
    windowed, wstats = device_likelihoods(problem)
    assert wstats["slot_runs"] == whole_stats["slot_runs"] and wstats["window"] < problem.n_variants // 3, wstats   # at least 3 windows
    assert np.array_equal(windowed, whole), np.abs(windowed - whole).max()


def test_two_solves_give_the_same_doubles():
    problem, _ = case("chain_single")
    first, stats = device_likelihoods(problem)
    second, _ = device_likelihoods(problem)
    assert stats["slot_runs"] > 0
    assert np.array_equal(first, second)
