"""GPU: comparing polyploid phasings (whatshap_amd.compare, csrc/polycompare_device.hip).  All recorded cases as one batch against the
recording and against compare_cases.dense_oracle, as tests/test_compare_host.py holds the host twin; the device against the one-thread
host twin of the debug library on every output, path included, totals as bit patterns; two medium cases the reference was not run on;
the number of launches of a call."""
import numpy as np
import pytest

import compare_cases as cc
from whatshap_amd import compare as cmp

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in cc.load_golden()["cases"]}
MAX_LAUNCHES = 2   # what the C ABI allows for; the kernel walks back in the launch of its forward pass (csrc/polycompare_device.hip)


def _batch(want_path=True):
    jobs, first = [], {}
    for name, case in CASES.items():
        first[name] = len(jobs)
        jobs += cc.jobs_of(case, want_path=want_path)
    return jobs, first


@pytest.fixture(scope="module")
def results():
    """All recorded cases as one batch on the device and through the host twin."""
    jobs, first = _batch()
    stats = []
    dev = cmp.switch_flips_batch(jobs, stats=stats)
    host = cmp.switch_flips_batch(jobs, host=True)
    assert 1 <= stats[0]["launches"] <= MAX_LAUNCHES and stats[0]["n_jobs"] == len(jobs)
    return dev, host, first


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_the_reference_and_the_canonical_split(name, results):
    dev, _, first = results
    cc.check_against_recording(CASES[name], dev[first[name]:first[name] + len(CASES[name]["costs"]) + 1])


def same(dev, host):
    assert np.float64(dev.total).view(np.uint64) == np.float64(host.total).view(np.uint64)
    for field in ("switches", "flips", "n_matched", "n_visited", "min_hamming_sum"):
        assert getattr(dev, field) == getattr(host, field), field
    assert (dev.positions is None) == (host.positions is None)
    if dev.positions is not None:
        for field in ("positions", "ranks", "perms", "flipped", "switches_in_column"):
            assert np.array_equal(getattr(dev, field), getattr(host, field)), field


def test_device_equals_the_host_twin_on_every_output(results):
    dev, host, _ = results
    assert len(dev) == len(host)
    for d, h in zip(dev, host):
        same(d, h)


def test_medium_cases_the_reference_was_not_run_on():
    cases = cc.medium_cases()
    assert [(c["ploidy"], len(c["phasing0"][0])) for c in cases] == [(6, 300), (5, 1000)]
    jobs = []
    for c in cases:
        jobs += [cmp.CompareJob(c["phasing0"], c["phasing1"], 1, 1, want_path=True),
                 cmp.CompareJob(c["phasing0"], c["phasing1"], 1, cc.switch_error_cost(c), matched_only=True, want_path=True)]
    stats = []
    dev = cmp.switch_flips_batch(jobs, stats=stats)
    host = cmp.switch_flips_batch(jobs, host=True)
    assert 1 <= stats[0]["launches"] <= MAX_LAUNCHES
    for d, h in zip(dev, host):
        same(d, h)
    for c, at in zip(cases, (0, 2)):
        p0, p1 = cc.arrays(c)
        matching = cc.matching_positions(p0, p1)
        assert 2 <= len(matching) < len(p0)
        for res, (sc, fc, pos) in zip(dev[at:at + 2], ((1, 1, range(len(p0))), (1, cc.switch_error_cost(c), matching))):
            assert (res.total, res.switches, res.flips) == cc.dense_oracle(p0[list(pos)], p1[list(pos)], sc, fc)
            cc.check_path(p0, p1, list(pos), sc, fc, res)
        assert dev[at].min_hamming_sum == cc.min_hamming_sum(p0, p1) and dev[at + 1].flips == 0


def test_launches_do_not_grow_with_the_batch():
    names = ["planted_p2_n64", "planted_p3_n65", "planted_p4_n91", "planted_p5_n89", "planted_p6_n70", "one_match_p6", "alleles_0_to_3_p4", "duplicates_p6"]
    jobs = [cmp.CompareJob(CASES[n]["phasing0"], CASES[n]["phasing1"], want_path=bool(x % 2)) for x, n in enumerate(names)]
    assert len(jobs) == 8 and {j.ploidy for j in jobs} == {2, 3, 4, 5, 6}
    stats = []
    res = cmp.switch_flips_batch(jobs, stats=stats)
    assert 1 <= stats[0]["launches"] <= MAX_LAUNCHES
    one = []
    cmp.switch_flips_batch(jobs[:1], stats=one)
    assert one[0]["launches"] == stats[0]["launches"]
    for n, r in zip(names, res):
        p0, p1 = cc.arrays(CASES[n])
        assert (r.total, r.switches, r.flips) == cc.dense_oracle(p0, p1)


def test_only_empty_jobs_no_device_work():
    none = CASES["no_match_p5"]
    jobs = [cmp.CompareJob([""] * 4, [""] * 4), cmp.CompareJob(none["phasing0"], none["phasing1"], 1, 99, matched_only=True, want_path=True),
            cmp.CompareJob([""] * 6, [""] * 6, want_path=True)]
    stats = []
    for res in cmp.switch_flips_batch(jobs, stats=stats):
        assert (res.total, res.switches, res.flips, res.n_visited, res.min_hamming_sum) == (0.0, 0, 0, 0, 0)
    assert stats[0]["launches"] == 0 and stats[0]["kernel_ms"] == 0 and stats[0]["upload_ms"] == 0


def test_a_path_job_beside_a_counts_only_job_returns_the_same_counts():
    for name in ("planted_p6_n65", "planted_p4_n91", "many_errors_p5", "one_match_p4"):
        c = CASES[name]
        with_path, without = cmp.switch_flips_batch([cmp.CompareJob(c["phasing0"], c["phasing1"], 2, 1, want_path=True),
                                                     cmp.CompareJob(c["phasing0"], c["phasing1"], 2, 1)])
        assert with_path.positions is not None and without.positions is None
        assert (with_path.total, with_path.switches, with_path.flips, with_path.min_hamming_sum) == (without.total, without.switches, without.flips, without.min_hamming_sum)


def test_compare_blocks_on_the_device():
    names = ["planted_p2_n90", "planted_p3_n90", "planted_p6_n64", "no_match_p3", "one_match_p6", "alleles_0_to_3_p6"]
    blocks = [(CASES[n]["phasing0"], CASES[n]["phasing1"]) for n in names]
    stats = []
    dev = cmp.compare_blocks(blocks, stats=stats)
    host = cmp.compare_blocks(blocks, host=True)
    assert stats[0]["n_jobs"] == 10 and 1 <= stats[0]["launches"] <= MAX_LAUNCHES   # two jobs per polyploid block, none for the diploid one
    for n, d, h in zip(names, dev, host):
        ref = CASES[n]["ref"]["block"]
        assert repr(d) == repr(h)
        assert (d.switches, d.hamming, d.diff_genotypes) == (ref["switches"], ref["hamming"], ref["diff_genotypes"])
