"""GPU: the polyphase threading DP on the device (csrc/polythreader_device.hip).  The same checks as tests/test_haplothread_host.py on
every recorded case -- (A) score, (B) the path's cost under the recurrence, (C) shape, (D) coverages and coverage costs, (E) the path
where ambiguous == 0 -- and device == host twin byte for byte: scores, paths, ambiguous, coverage costs.  The launch count does not
depend on the batch."""
import numpy as np
import pytest

import haplothread_cases as hc
from whatshap_amd import _native, polythread

pytestmark = pytest.mark.gpu

GOLDEN = hc.load_golden()
CASES = GOLDEN["cases"]
BY_NAME = {c["name"]: c for c in CASES}


@pytest.fixture(scope="module")
def results():
    problems = [hc.problem_of(c) for c in CASES]
    return polythread.thread_batch(problems), polythread.thread_batch(problems, host=True)


@pytest.mark.parametrize("k", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_case_against_the_reference_and_the_twin(results, k):
    device, twin = results
    hc.check_case(CASES[k], device[k])
    for name in polythread.ThreadingResult.ARRAYS:
        assert np.array_equal(getattr(device[k], name).view(np.uint8), getattr(twin[k], name).view(np.uint8)), (CASES[k]["name"], name)
    assert device[k].tobytes() == twin[k].tobytes()
    for key in ("n_positions", "n_sections", "n_tuples", "n_entries"):
        assert device[k].stats[key] == twin[k].stats[key], key


def test_at_least_half_of_the_random_cases_of_every_ploidy_are_unambiguous(results):
    device, _ = results
    for p in hc.PLOIDIES:
        mine = [k for k, c in enumerate(CASES) if c["name"].startswith(f"random_p{p}_")]
        assert len(mine) == hc.RANDOM_PER_PLOIDY[p]
        unique = sum(1 for k in mine if not device[k].ambiguous.any())
        assert 2 * unique >= len(mine), (p, unique, len(mine))


def test_the_launch_count_does_not_depend_on_the_batch(results):
    device, _ = results
    assert all(r.stats["launches"] == _native.POLY_THREADER_LAUNCHES == 5 for r in device)
    alone = polythread.thread_batch([hc.problem_of(BY_NAME["one_position"])])[0]
    assert alone.stats["launches"] == 5
    assert polythread.thread_batch([])== []


def test_a_batch_of_mixed_ploidies_and_lengths_equals_the_calls_one_by_one(results):
    device, _ = results
    picked = [k for k, c in enumerate(CASES) if c["name"] in ("random_p2_s2000", "full_6_8_shallow", "sections", "random_p5_s5003", "one_position", "gap_0", "random_p4_s4001")]
    assert len(picked) == 7
    for k in picked:
        alone = polythread.thread_batch([hc.problem_of(CASES[k])])[0]
        assert alone.tobytes() == device[k].tobytes(), CASES[k]["name"]


def test_the_pipeline_cases_and_the_references_signature(results):
    for rec in GOLDEN["pipeline"][::3]:
        res = polythread.thread_batch([hc.problem_of(rec)])[0]
        hc.check_case(rec, res)
    c = BY_NAME["readded_empty_rows"]
    cov_map, allele_depths = hc.dicts_of(c)
    assert polythread.compute_threading_path(cov_map, allele_depths, c["ploidy"], c["switch_cost"], c["affine_switch_cost"], c["max_gap"]) == c["path"]


def test_refusals_launch_nothing():
    c = BY_NAME["random_p3_s3000"]
    for changes, match in ((dict(ploidy=7), "ploidy 7 outside 2 .. 6"), (dict(switch_cost=0.1, affine_switch_cost=0.1), "not exact in float"),
                           (dict(block_starts=[2]), "block_starts must begin with 0")):
        with pytest.raises(ValueError, match=match):
            polythread.thread_batch([hc.problem_of(dict(c, **changes))])
    with pytest.raises(ValueError, match="row_limit 8: only 0"):
        polythread.thread_batch([hc.problem_of(c, row_limit=8)])
    with pytest.raises(IndexError, match="has no depth row"):
        polythread.thread_batch([hc.problem_of(dict(c, depths=[[]] + c["depths"][1:]))])


def test_run_threading_on_the_device_equals_the_twin():
    import polythread_cases as pc

    recorded = pc.load_golden()["cases"]
    for rec in GOLDEN["pipeline"][::5]:
        case = recorded[rec["index"]]
        matrix = pc.problem_of(case).matrix
        got = polythread.run_threading(matrix, case["clustering"], case["ploidy"], [], True, case["max_gap"])
        assert got == polythread.run_threading(matrix, case["clustering"], case["ploidy"], [], True, case["max_gap"], host=True)
        assert len(got[0]) == case["n_pos"] and len(got[1]) == case["ploidy"]
