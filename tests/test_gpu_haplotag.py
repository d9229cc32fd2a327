"""GPU: haplotagging (whatshap_amd.haplotag, csrc/haplotag_device.hip) against every recorded reference case and, on problems the
reference was not run on, against the one-thread host twin of the debug library: identical in every field, the counts of the stats included."""
import numpy as np
import pytest

import haplotag_cases as hc
from whatshap_amd import haplotag as ht

pytestmark = pytest.mark.gpu

GOLDEN = {c["spec"]["name"]: c for c in hc.load_golden()["cases"]}
SPECS = {s["name"]: s for s in hc.all_specs()}
COUNTS = ("n_reads", "n_groups", "n_assigned", "n_multiple_phase_sets", "n_entries", "groups_class_a", "groups_class_b", "groups_class_c", "groups_many_phase_sets")
A_MAX, B_MAX, SEGMENT, R = 64, 4096, 8, 4   # csrc/haplotag.h


def same(got, want):
    for field in ("haplotype", "quality", "phaseset", "bx", "bx_start", "bx_haplotype", "bx_phaseset"):
        assert np.array_equal(getattr(got, field), getattr(want, field)), field
    assert {k: got.stats[k] for k in COUNTS} == {k: want.stats[k] for k in COUNTS}


def device_and_host(problems):
    dev = ht.haplotag_batch(problems)
    host = ht.haplotag_batch(problems, host=True)
    for d, h in zip(dev, host):
        same(d, h)
    return dev


def test_device_equals_the_reference_on_every_recorded_case():
    for name, spec in SPECS.items():
        if spec["expect_error"]:
            continue
        data = hc.materialize(spec)
        got = hc.canonical(ht.prepare_haplotag_information(*hc.call_args(spec, data)))
        assert got == GOLDEN[name]["results"], name
        assert got == hc.canonical(ht.prepare_haplotag_information(*hc.call_args(spec, data), host=True)), name


BOUNDARY_LENGTHS = [0, 1, 2, SEGMENT - 1, SEGMENT, SEGMENT + 1, 63, 64, 65, 127, 128, 129, A_MAX - 1, A_MAX, A_MAX + 1, B_MAX - 1, B_MAX, B_MAX + 1, 50_021, 3, 0, 17]


@pytest.mark.parametrize("ploidy", [2, 3, 16])
@pytest.mark.parametrize("n_phasesets", [R - 1, R, R + 1])
def test_group_sizes_and_phase_set_counts_at_every_boundary(ploidy, n_phasesets):
    """Every read is a group; a read of L >= n_phasesets variants meets n_phasesets phase sets (one window: variant i belongs to set i mod n)."""
    p = hc.array_problem(ploidy, BOUNDARY_LENGTHS, seed=11 * ploidy + n_phasesets, n_phasesets=n_phasesets, n_variants=60_000, window=60_000)
    s = device_and_host([p])[0].stats
    assert s["launches"] == 3
    assert s["groups_class_a"] > 0 and s["groups_class_b"] > 0 and s["groups_class_c"] > 0
    if n_phasesets > R:
        assert s["groups_many_phase_sets"] >= 10   # in every class
    else:
        assert s["groups_many_phase_sets"] == 0


@pytest.mark.parametrize("ploidy", [2, 3, 16])
def test_waves_of_a_workgroup_that_meet_different_phase_sets(ploidy):
    """One workgroup per long group: every wave's quarter of the run has at most R phase sets of its own, all quarters together have more
    (windows of 6 000 variants, two sets each); and quarters that share theirs (one window)."""
    few = hc.array_problem(ploidy, [19_990, 5, 19_000], seed=5, n_phasesets=2, n_variants=40_000, window=6_000)
    shared = hc.array_problem(ploidy, [30_000, 4_097], seed=6, n_phasesets=R, n_variants=40_000, window=40_000)
    dev = device_and_host([few, shared])
    assert dev[0].stats["groups_class_c"] == 2 and dev[0].stats["groups_many_phase_sets"] == 2
    assert dev[1].stats["groups_class_c"] == 2 and dev[1].stats["groups_many_phase_sets"] == 0


def test_large_random_problem_with_a_heavy_tail():
    lengths = hc.heavy_tail_lengths(200_000, seed=21, tail_max=20_000)
    p = hc.array_problem(2, lengths, seed=22, n_phasesets=3, n_variants=80_000, window=64)
    s = device_and_host([p])[0].stats
    assert s["n_reads"] == 200_000 and s["groups_class_a"] > 150_000 and s["groups_class_b"] > 1_000 and s["groups_class_c"] > 10
    assert s["groups_many_phase_sets"] > 100 and s["n_multiple_phase_sets"] > 100_000 and s["launches"] == 3


def test_linked_reads_on_the_device():
    rng = np.random.default_rng(31)
    p = hc.array_problem(4, rng.integers(0, 4, size=30_000), seed=32, n_variants=20_000, linked=(1_500, 40_000))
    s = device_and_host([p])[0].stats
    assert s["n_groups"] < 30_000 and s["n_assigned"] > 1_000


def test_a_batch_equals_its_problems_one_by_one_and_takes_no_more_launches():
    rng = np.random.default_rng(41)
    problems = []
    for k in range(300):
        if k == 17:
            lengths = []                       # an empty problem
        elif k == 40:
            lengths = [0, 0, 0]                # only empty reads
        else:
            lengths = rng.integers(0, 4 if k % 5 == 0 else 40, size=int(rng.integers(1, 30)))   # (every group stays within 64 entries: one class, one launch)
        problems.append(hc.array_problem((2, 3, 4, 16)[k % 4], lengths, seed=100 + k, n_variants=300, linked=(3, 20_000) if k % 5 == 0 else None))
    batch = device_and_host(problems)
    single_launches = None
    for k, p in enumerate(problems):
        alone = ht.haplotag_batch([p])[0]
        same(batch[k], alone)
        if k == 0:
            single_launches = alone.stats["launches"]
        assert alone.stats["launches"] == (0 if k in (17, 40) else 1)
    assert single_launches == 1 and all(b.stats["launches"] == single_launches for b in batch)


def test_calls_without_device_work_launch_nothing():
    empty = hc.array_problem(2, [], seed=1)
    hollow = hc.array_problem(3, [0, 0, 0, 0], seed=2, linked=(2, 10))
    for problems in ([], [empty], [hollow], [empty, hollow, empty]):
        for res in ht.haplotag_batch(problems):
            assert res.stats["launches"] == 0 and res.stats["n_assigned"] == 0 and (res.haplotype == -1).all()
    assert ht.haplotag_batch([hollow])[0].stats["n_groups"] >= 1
