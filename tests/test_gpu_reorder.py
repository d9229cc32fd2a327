"""GPU: polyphase reordering (whatshap_amd.reorder, csrc/polyreorder_device.hip) against every recorded reference case -- link log
likelihoods bit for bit, windows, chosen permutations, assignments, threads and haplotypes equal, confidences within the bound of
reorder_cases.check_against_recording -- and, on a problem the reference was not run on, against the one-thread host twin of the debug
library bit for bit; the number of launches of a call."""
import numpy as np
import pytest

import reorder_cases as rc
from whatshap_amd import reorder as ro

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in rc.load_golden()["cases"]}
MAX_LAUNCHES = 2   # the table kernel and the permutation kernel (csrc/polyreorder_device.hip)


@pytest.fixture(scope="module")
def device_results():
    """All recorded cases as one batch on the device, fed the recorded cluster order."""
    stats = []
    res = ro.link_likelihoods_batch([rc.problem(c, rc.recorded_clusters(c)) for c in CASES.values()], stats=stats)
    assert all(s["launches"] == MAX_LAUNCHES for s in stats)
    return dict(zip(CASES, res))


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_the_reference(name, device_results):
    rc.check_against_recording(CASES[name], device_results[name])


def same(dev, host):
    assert dev.llh_flat.view(np.uint64).tolist() == host.llh_flat.view(np.uint64).tolist()
    assert dev.windows == host.windows and dev.best.tolist() == host.best.tolist()
    for field in ("assignments", "threads", "haplotypes"):
        assert np.array_equal(getattr(dev, field), getattr(host, field)), field
    assert dev.confidence.view(np.uint64).tolist() == host.confidence.view(np.uint64).tolist()   # (the same llh through the same host exp)


def test_device_equals_the_host_twin_on_a_medium_case():
    case = rc.medium_case()
    assert case["ploidy"] == 6 and case["n_pos"] == 300 and len(case["reads"]) >= 600 and len(case["breakpoints"]) >= 10
    assert max(len(b[1]) for b in case["breakpoints"]) >= 4
    dev_stats, host_stats = [], []
    dev = ro.link_likelihoods_batch([rc.problem(case)], stats=dev_stats)[0]
    host = ro.link_likelihoods_batch([rc.problem(case)], host=True, stats=host_stats)[0]
    same(dev, host)
    counts = ("n_breakpoints", "n_reads_visited", "n_permutations", "n_window_positions")
    assert {k: dev_stats[0][k] for k in counts} == {k: host_stats[0][k] for k in counts}
    assert dev_stats[0]["launches"] == MAX_LAUNCHES and host_stats[0]["launches"] == 0


def test_launches_do_not_grow_with_the_batch():
    names = ["random_p2_find_1", "random_p4_subsets_11", "zero_breakpoints", "lds_tile", "seven_of_eight", "span_edges", "random_p6_find_13", "duplicate_haplotypes"]
    stats = []
    res = ro.link_likelihoods_batch([rc.problem(CASES[n], rc.recorded_clusters(CASES[n])) for n in names], stats=stats)
    assert len(res) == 8 and [s["launches"] for s in stats] == [MAX_LAUNCHES] * 8
    for n, r in zip(names, res):
        rc.check_against_recording(CASES[n], r)


def test_no_breakpoints_no_device_work():
    case = CASES["zero_breakpoints"]
    stats = []
    res = ro.link_likelihoods_batch([rc.problem(case, [])] * 3, stats=stats)
    assert [s["launches"] for s in stats] == [0, 0, 0] and all(s["kernel_ms"] == 0 and s["upload_ms"] == 0 for s in stats)
    for r in res:
        assert r.threads.tolist() == case["threads"] and r.haplotypes.tolist() == case["haplotypes"] and r.assignments.tolist() == [[0, 1, 2]]
