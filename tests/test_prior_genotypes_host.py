"""CPU: the prior genotype likelihoods (whatshap_amd.genotype.compute_genotypes and friends, csrc/priorgt.cpp) through the one-thread
host twin of the debug library -- the same chain and tail functions the kernel calls -- against every value recorded from the reference:
float.hex for float.hex, no tolerance; the refusals; the Python-level functions; a batch against its problems alone."""
import numpy as np
import pytest

import prior_genotype_cases as pc
from whatshap_amd import _native, core
from whatshap_amd import genotype as gt

GOLDEN = pc.load_golden()
BY_NAME = {c["name"]: c for c in GOLDEN}


def hexes(array):
    return [pc.hex3(row) for row in array.tolist()]


def check_against_golden(case, res):
    name = case["name"]
    assert hexes(res.gl) == case["gl"], name
    assert res.genotype.tolist() == case["gt"], name
    if case["constant"] is not None:
        assert hexes(res.reg) == case["reg"], name
        assert res.reg_genotype.tolist() == case["reg_gt"], name
    else:
        assert not res.reg.any() and (res.reg_genotype == -1).all(), name


def test_the_fixture_covers_what_it_is_meant_to():
    names = set(BY_NAME)
    assert {f"run_{n}" for n in pc.BOUNDARY_RUNS} <= names and len([n for n in names if n.startswith("random_")]) == 40
    assert BY_NAME["deep_ref_q30"]["gl"][0] == pc.hex3((1.0, 1e-323, 0.0))   # a subnormal
    assert BY_NAME["no_positions"]["gl"] == [] and BY_NAME["no_reads"]["gt"] == [-1, -1, -1]
    assert BY_NAME["no_reads"]["gl"] == [pc.hex3((1 / 3, 1 / 3, 1 / 3))] * 3
    assert any(c["positions"] is None for c in GOLDEN)
    # a column whose two largest regularised values tie has no genotype, whatever the threshold
    tie = BY_NAME["grid_c0.5_t0"]
    assert tie["reg"][1][0] == tie["reg"][1][1] == tie["reg"][1][2] and tie["reg_gt"][1] == -1
    seen = {(c["constant"], c["gt_qual_threshold"]) for c in GOLDEN if c["constant"] is not None}
    assert {(c, t) for c in pc.CONSTANTS for t in pc.THRESHOLDS} <= seen
    assert any(g >= 0 for c in GOLDEN if c["constant"] is not None for g in c["reg_gt"])


def test_host_twin_equals_every_recorded_value():
    results = gt.prior_genotypes_batch([pc.problem_of(c) for c in GOLDEN], host=True)
    for case, res in zip(GOLDEN, results):
        check_against_golden(case, res)
        assert res.stats["launches"] == 0   # (the host twin launches nothing)
        counted = sum(len(col) for col in pc.columns_of(case))
        assert res.stats["n_counted"] == counted and res.stats["n_positions"] == len(case["gl"])


def test_factor_codes_cover_every_quality():
    """One entry per column: quality q and min(q, 14) give the same bits from 14 on, and every smaller one its own."""
    for allele in (0, 1):
        reads = [[(q, allele, q)] for q in range(0, 100)]
        res = gt.prior_genotypes_batch([pc.problem_of(pc.from_reads("q", reads, list(range(100))))], host=True)[0]
        want = [pc.hex3(pc.python_chain([(allele, q)])) for q in range(100)]
        assert hexes(res.gl) == want
        assert len({tuple(w) for w in want}) == 15


def refused(reads, positions):
    with pytest.raises(ValueError) as err:
        gt.prior_genotypes_batch([pc.problem_of(pc.from_reads("bad", reads, positions))], host=True)
    return str(err.value)


def test_the_four_refusals_name_the_read():
    ok = [(10, 0, 30), (20, 1, 30)]
    assert "read 2" in refused([ok, ok, [(5, 0, 30), (20, 0, 30)]], [5, 10, 20])           # starts before the read in front of it
    assert "not sorted" in refused([ok, [(5, 0, 30)]], [5, 10, 20])
    message = refused([ok, [(10, 0, 30), (30, 1, 30), (20, 0, 30)]], [10, 20, 30])          # positions not strictly increasing
    assert "read 1" in message and "strictly increasing" in message
    assert "read 1" in refused([ok, [(10, 0, 30), (10, 1, 30)]], [10, 20])
    message = refused([ok, [(15, 0, 30), (20, 1, 30)]], [10, 20])                           # first position not in the list
    assert "read 1" in message and "first position" in message
    message = refused([ok, ok, ok, [(10, 0, 30), (25, 1, 30)]], [10, 20])                   # last position not in the list
    assert "read 3" in message and "last position" in message
    assert "duplicate" in refused([ok], [10, 20, 20])
    assert "read 0" in refused([[]], [10])                                                  # (firstPosition() of an empty read)
    # the reference's iterator walks the list front to back: a list that is not sorted is refused as well
    assert "strictly increasing" in refused([ok], [20, 10])
    # inside a batch the problem is named too
    with pytest.raises(ValueError, match="problem 1: read 0"):
        gt.prior_genotypes_batch([pc.problem_of(pc.from_reads("a", [ok], [10, 20])), pc.problem_of(pc.from_reads("b", [[(15, 0, 1)]], [10]))], host=True)


def test_entries_between_listed_positions_are_passed_over():
    reads = [[(10, 0, 30), (12, 1, 30), (14, 1, 1), (20, 1, 30)], [(10, 1, 5), (13, 0, 5), (20, 3, 5)]]
    res = gt.prior_genotypes_batch([pc.problem_of(pc.from_reads("gaps", reads, [10, 11, 20, 400]))], host=True)[0]
    want = [pc.python_chain(e) for e in ([(0, 30), (1, 5)], [], [(1, 30)], [])]
    assert hexes(res.gl) == [pc.hex3(w) for w in want]
    assert res.stats["n_counted"] == 3 and res.stats["n_covered"] == 2


def test_compute_genotypes_returns_the_references_types_and_values():
    for name in ("random_1000", "random_1004", "random_1007", "run_65", "no_reads", "no_positions", "none_counted"):
        case = BY_NAME[name]
        genotypes, gls = gt.compute_genotypes(pc.readset_of(case, core), case["positions"], host=True)
        assert all(isinstance(g, core.Genotype) for g in genotypes) and all(isinstance(g, tuple) and len(g) == 3 for g in gls)
        assert [pc.hex3(g) for g in gls] == case["gl"], name
        assert genotypes == [gt.int_to_diploid_biallelic_gt(g) for g in case["gt"]], name
        assert [g.is_none() for g in genotypes] == [g < 0 for g in case["gt"]]


def test_prior_likelihoods_fuses_the_regularisation():
    for case in GOLDEN:
        if case["constant"] is None or not case["name"].startswith(("grid_", "random_1000", "no_reads")):
            continue
        genotypes, reg = gt.prior_likelihoods(pc.readset_of(case, core), case["positions"], case["constant"], case["gt_qual_threshold"], host=True)
        assert all(isinstance(r, core.PhredGenotypeLikelihoods) for r in reg)
        assert [pc.hex3(r.as_vector()) for r in reg] == case["reg"], case["name"]
        assert genotypes == [gt.int_to_diploid_biallelic_gt(g) for g in case["reg_gt"]], case["name"]
        # determine_genotype on the host gives the same answer from the likelihoods
        assert [gt.determine_genotype(r, pc.gt_prob_of(case)) for r in reg] == genotypes


def test_determine_genotype():
    assert gt.determine_genotype([0.1, 0.7, 0.2], 0.5) == core.Genotype([0, 1])
    assert gt.determine_genotype([0.1, 0.7, 0.2], 0.7).is_none()            # not strictly above the threshold
    assert gt.determine_genotype([0.45, 0.45, 0.1], 0.0).is_none()          # the two largest tie
    assert gt.determine_genotype(core.PhredGenotypeLikelihoods([0.0, 0.25, 0.75]), 0.5) == core.Genotype([1, 1])
    assert gt.determine_genotype((0.9, 0.05, 0.05), 0.0) == core.Genotype([0, 0])


def test_a_batch_equals_its_problems_alone():
    cases = pc.fresh_batch(3, 8)
    problems = [pc.problem_of(c) for c in cases]
    batch = gt.prior_genotypes_batch(problems, host=True)
    for case, p, together in zip(cases, problems, batch):
        alone = gt.prior_genotypes_batch([p], host=True)[0]
        for field in ("gl", "genotype", "reg", "reg_genotype"):
            assert getattr(alone, field).tobytes() == getattr(together, field).tobytes(), (case["name"], field)
        assert hexes(alone.gl) == [pc.hex3(pc.python_chain(e)) for e in pc.columns_of(case)]


def test_bindings_mirror_the_header():
    import os
    import re

    header = open(os.path.join(os.path.dirname(os.path.abspath(_native.__file__)), "..", "include", "whatshap_amd.h")).read()
    assert int(re.search(r"#define WHAMD_PRIOR_GENOTYPES_LAUNCHES (\d+)u", header).group(1)) == _native.PRIOR_GENOTYPES_LAUNCHES
    assert 8 * 7 + np.dtype(np.float64).itemsize * 2 + 4 * 2 == __import__("ctypes").sizeof(_native.PriorGenotypesView)   # seven words, two doubles, two uint32


def test_the_references_own_readset_goes_through_the_compiled_ingestion():
    """compute_genotypes on whatshap.core.ReadSet objects, and the shim's replacement handing back the reference's Genotype class."""
    import refobjects
    from whatshap_amd import ingest

    ref = refobjects.reference_core()
    assert ingest.load() is not None
    for name in ("random_1002", "random_1004", "grid_c0.001_t10"):
        case = BY_NAME[name]
        readset = pc.readset_of(case, ref)
        genotypes, gls = gt.compute_genotypes(readset, case["positions"], host=True)
        assert [pc.hex3(g) for g in gls] == case["gl"], name
        assert [sum(g.as_vector()) if not g.is_none() else -1 for g in genotypes] == case["gt"], name
        # ... and equal to what the reference itself returns for the same object
        ref_genotypes, ref_gls = ref.compute_genotypes(readset, case["positions"])
        assert [pc.hex3(g) for g in ref_gls] == [pc.hex3(g) for g in gls]
        assert [sorted(g.as_vector()) for g in ref_genotypes] == [g.as_vector() for g in genotypes]


@pytest.mark.skipif(_native.device_count() > 0, reason="only meaningful on a machine without a GPU")
def test_without_a_device_the_native_call_raises():
    with pytest.raises(_native.SolverError) as e:
        gt.prior_genotypes_batch([pc.problem_of(BY_NAME["random_1000"])])
    assert e.value.status == _native.WHAMD_ERR_DEVICE
    # a refusal comes first, and a call without a counted entry never opens the device
    with pytest.raises(ValueError, match="read 0"):
        gt.prior_genotypes_batch([pc.problem_of(pc.from_reads("bad", [[(15, 0, 1)]], [10]))])
    assert gt.prior_genotypes_batch([pc.problem_of(BY_NAME["no_reads"])])[0].stats["launches"] == 0


def test_the_new_exports_follow_the_export_rule():
    import subprocess

    names = [n for n in _native.EXPORTED_SYMBOLS if n.startswith("whamd_prior_genotypes")]
    assert len(names) == 6
    for path, debug in ((_native.LIB_PATH, False), (_native.DEBUG_LIB_PATH, True)):
        exported = {ln.split()[-1] for ln in subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout.splitlines() if ln.strip()}
        assert set(names) <= exported
        assert ("whamd_debug_prior_genotypes_host" in exported) == debug
