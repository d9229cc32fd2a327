"""GPU: the read merging on the device against what the reference's ReadMerger.merge recorded and, field for field, against the host
twin; all cases as one batch in one call with the launch constant; two calls byte for byte; merge -> readselection -> PedigreeDPTable."""
import numpy as np
import pytest

import readmerge_cases as rc
from helpers import biallelic_gt
from test_readmerge_host import GOLDEN, SPECS, case_ids, check_case
from whatshap_amd import readmerge as rm
from whatshap_amd.core import NumericSampleIds, Pedigree, PedigreeDPTable, Read, ReadSet
from whatshap_amd.readselect import readselection

pytestmark = pytest.mark.gpu

ALL_FIELDS = rm.MergeResult.FIELDS + rm.MergeResult.EDGE_FIELDS
COUNTS = ("n_reads", "n_entries", "n_pairs", "n_blue", "n_not_blue", "n_merged_components", "n_merged_entries", "n_super_entries")


def problems_of_all_cases():
    usable = [c for c in GOLDEN if not c["raises"]]
    problems = []
    for c in usable:
        spec = SPECS[c["spec"]["name"]]
        problems.append(rm.MergeProblem.from_readset(rc.readset_of(rc.materialize(spec)), *rm.thresholds(spec["error_rate"], spec["positive_threshold"], spec["negative_threshold"]),
                                                     spec["max_error_rate"]))
    return usable, problems


@pytest.mark.parametrize("record", GOLDEN, ids=case_ids())
def test_device_equals_the_reference_and_the_host_twin(record):
    res = check_case(record, host=False)
    if res is None:   # the case raises before any native call
        return
    spec = SPECS[record["spec"]["name"]]
    problem = rm.MergeProblem.from_readset(rc.readset_of(rc.materialize(spec)), *rm.thresholds(spec["error_rate"], spec["positive_threshold"], spec["negative_threshold"]),
                                           spec["max_error_rate"])
    device_stats, host_stats = [], []
    on_device = rm.merge_batch([problem], want_edges=True, stats=device_stats)[0]
    on_host = rm.merge_batch([problem], host=True, want_edges=True, stats=host_stats)[0]
    for name in ALL_FIELDS:
        a, b = getattr(on_device, name), getattr(on_host, name)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name
    for name in COUNTS:
        assert device_stats[0][name] == host_stats[0][name], name
    pairs, merged = device_stats[0]["n_pairs"] > 0, device_stats[0]["n_merged_entries"] > 0
    assert device_stats[0]["launches"] == 4 * pairs + 5 * merged and host_stats[0]["launches"] == 0


def test_all_cases_as_one_batch_in_one_call():
    usable, problems = problems_of_all_cases()
    device_stats = []
    batch = rm.merge_batch(problems, want_edges=True, stats=device_stats)
    assert all(s["launches"] == rm.LAUNCHES == 9 for s in device_stats)
    twin = rm.merge_batch(problems, host=True, want_edges=True)
    for c, got, want in zip(usable, batch, twin):
        for name in ALL_FIELDS:
            assert getattr(got, name).tobytes() == getattr(want, name).tobytes(), (c["spec"]["name"], name)
        assert [list(e[:4]) for e in sorted(got.edges(), key=lambda e: (e[1], e[0]))] == c["results"]["blue"]
    # a different batch, the same constant
    few = rm.merge_batch(problems[:3], want_edges=True, stats=device_stats)
    assert device_stats[-1]["launches"] == rm.LAUNCHES and few[2].edge_j.tobytes() == batch[2].edge_j.tobytes()


def test_two_calls_on_one_input_are_byte_for_byte_the_same():
    _, problems = problems_of_all_cases()
    first = rm.merge_batch(problems, want_edges=True)
    second = rm.merge_batch(problems, want_edges=True)
    for a, b in zip(first, second):
        for name in ALL_FIELDS:
            assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name


def test_a_larger_sorted_read_set_equals_the_host_twin():
    """More than one workgroup of pairs and more than one tile of the scan: 3 000 reads of the benchmark's read set."""
    read_ptr, position, allele, quality = rc.bench_reads(n_variants=6000, coverage=20, seed=3)
    problem = rm.MergeProblem(read_ptr, position, allele, quality, 5, 3, 0.25)
    device_stats = []
    got = rm.merge_batch([problem], want_edges=True, stats=device_stats)[0]
    want = rm.merge_batch([problem], host=True, want_edges=True)[0]
    assert device_stats[0]["n_pairs"] > 4096 and device_stats[0]["n_blue"] > 0 and device_stats[0]["launches"] == rm.LAUNCHES
    for name in ALL_FIELDS:
        assert getattr(got, name).tobytes() == getattr(want, name).tobytes(), name


def phase(readset):
    """select_reads and the table, as cli/phase.py runs them after the merging."""
    readset.sort()
    selected = readset.subset(readselection(readset, 15))
    positions = sorted({v.position for read in selected for v in read})
    pedigree = Pedigree(NumericSampleIds())
    pedigree.add_individual("individual0", [biallelic_gt(1)] * len(positions))
    table = PedigreeDPTable(selected, [1] * len(positions), pedigree)
    superreads, transmission = table.get_super_reads()
    return (table.get_optimal_cost(), table.get_optimal_partitioning(), [rc.canonical_reads(rs) for rs in superreads], transmission,
            rc.canonical_reads(selected))


def test_merge_then_select_then_table_equals_the_chain_fed_with_the_recorded_merged_reads():
    record = next(c for c in GOLDEN if c["spec"]["name"] == "phase_input")
    spec = SPECS["phase_input"]
    data = rc.materialize(spec)
    assert all(len(read) >= 2 for read in data["reads"])   # cli/phase.py:518-520 keeps only such reads in front of the merging
    merged = rm.ReadMerger(*rc.merger_args(spec)).merge(rc.readset_of(data))
    recorded = ReadSet()
    for name, variants in record["results"]["merged"]:
        read = Read(name)
        for position, allele, quality in variants:
            read.add_variant(position, allele, quality)
        recorded.add(read)
    assert 2 < len(recorded) < len(data["reads"])   # something was merged, something was not
    assert phase(merged) == phase(recorded)
