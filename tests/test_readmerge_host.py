"""CPU: the read merging (whatshap_amd.readmerge) on the one-thread host twin of the debug library against what the reference's
ReadMerger.merge recorded (tests/golden/readmerge_cases.json.gz): edges, representatives, superreads, merged reads, exception classes;
and the array-level checks of the native call -- mismatched lengths, every refusal, no launch on the host, representatives given."""
import numpy as np
import pytest

import readmerge_cases as rc
from whatshap_amd import _native, readmerge as rm

try:
    import networkx  # noqa: F401
    HAVE_NETWORKX = True
except ImportError:
    HAVE_NETWORKX = False

GOLDEN = rc.load_golden()["cases"]
SPECS = {s["name"]: s for s in rc.all_specs()}
# the only cases a test may leave out, and only where networkx is missing: those whose components the removal loop has to cut
NEEDS_NETWORKX = sorted(c["spec"]["name"] for c in GOLDEN if not c["raises"] and c["results"]["not_blue"])


def case_ids():
    return [c["spec"]["name"] for c in GOLDEN]


def check_case(record, host, device=0):
    """One recorded case through merge_batch and ReadMerger: every recorded field."""
    spec = SPECS[record["spec"]["name"]]
    data = rc.materialize(spec)
    assert rc.input_sha256(data) == record["input_sha256"], "the generator drifted: regenerate the golden file"
    merger = rm.ReadMerger(*rc.merger_args(spec), host=host, device=device)
    if record["raises"]:
        with pytest.raises(Exception) as e:
            merger.merge(rc.readset_of(data))
        assert type(e.value).__name__ == record["raises"] == spec["expect_error"]
        return
    want = record["results"]
    thr_diff, thr_neg_diff = rm.thresholds(spec["error_rate"], spec["positive_threshold"], spec["negative_threshold"])
    problem = rm.MergeProblem.from_readset(rc.readset_of(data), thr_diff, thr_neg_diff, spec["max_error_rate"])
    stats = []
    res = rm.merge_batch([problem], host=host, device=device, want_edges=True, stats=stats)[0]
    edges = res.edges()
    assert edges == sorted(edges, key=lambda e: (e[0], e[1])) and len({e[:2] for e in edges}) == len(edges)
    in_reference_order = sorted(edges, key=lambda e: (e[1], e[0]))
    assert [list(e[:4]) for e in in_reference_order] == want["blue"]
    assert [list(e[:4]) for e in in_reference_order if e[4]] == want["not_blue"]
    assert stats[0]["n_blue"] == len(want["blue"]) and stats[0]["n_not_blue"] == len(want["not_blue"])
    assert stats[0]["n_reads"] == len(data["reads"]) and stats[0]["n_entries"] == sum(len(r) for r in data["reads"])
    if want["not_blue"]:
        if not HAVE_NETWORKX:
            pytest.skip(f"networkx is missing: {record['spec']['name']} needs the removal loop")
        representative = rm.cut_components(problem.n_reads, edges)
        res = rm.merge_batch([problem.with_representative(representative)], host=host, device=device)[0]
    assert res.representative.tolist() == want["representative"]
    sizes = np.bincount(np.asarray(want["representative"], dtype=np.int64), minlength=problem.n_reads)
    assert res.component_size.tolist() == [int(sizes[r]) for r in want["representative"]]
    got = [[f"read{k}", [list(v) for v in variants]] for k, variants in res.merged_reads(problem)]
    assert got == want["merged"]
    # the sums behind every superread entry
    for k in range(int(res.super_ptr[-1])):
        z0, z1 = int(res.sum0[k]), int(res.sum1[k])
        assert int(res.allele[k]) == (0 if z0 >= z1 else 1) and int(res.quality[k]) == abs(z1 - z0)
    merged = merger.merge(rc.readset_of(data))
    assert rc.canonical_reads(merged) == want["merged"]
    return res


def test_the_recorded_cases_are_the_generated_ones():
    assert case_ids() == [s["name"] for s in rc.all_specs()]
    assert len(NEEDS_NETWORKX) >= 2 and {"not_blue_cuts_a_component", "not_blue_between_components"} <= set(NEEDS_NETWORKX)


@pytest.mark.parametrize("record", GOLDEN, ids=case_ids())
def test_host_twin_equals_the_reference(record):
    check_case(record, host=True)


def test_the_host_twin_launches_nothing_and_the_batch_equals_the_single_calls():
    usable = [c for c in GOLDEN if not c["raises"]]
    problems = []
    for c in usable:
        spec = SPECS[c["spec"]["name"]]
        problems.append(rm.MergeProblem.from_readset(rc.readset_of(rc.materialize(spec)), *rm.thresholds(spec["error_rate"], spec["positive_threshold"], spec["negative_threshold"]),
                                                     spec["max_error_rate"]))
    stats = []
    batch = rm.merge_batch(problems, host=True, want_edges=True, stats=stats)
    assert all(s["launches"] == 0 for s in stats)
    for c, p, got in zip(usable, problems, batch):
        alone = rm.merge_batch([p], host=True, want_edges=True)[0]
        for name in rm.MergeResult.FIELDS + rm.MergeResult.EDGE_FIELDS:
            assert np.array_equal(getattr(got, name), getattr(alone, name)), (c["spec"]["name"], name)
        assert [list(e[:4]) for e in sorted(got.edges(), key=lambda e: (e[1], e[0]))] == c["results"]["blue"]


def test_representative_given_skips_pairs_and_components():
    data = rc.materialize(SPECS["chain"])
    problem = rm.MergeProblem.from_readset(rc.readset_of(data), 5, 3, 0.25)
    free = rm.merge_batch([problem], host=True, want_edges=True)[0]
    assert free.representative.tolist() == [0] * 7
    stats = []
    given = rm.merge_batch([problem.with_representative([0, 0, 2, 2, 2, 5, 6])], host=True, want_edges=True, stats=stats)[0]
    assert stats[0]["n_pairs"] == 0 and stats[0]["n_blue"] == 0 and given.edge_j.size == 0
    assert given.representative.tolist() == [0, 0, 2, 2, 2, 5, 6] and given.component_size.tolist() == [2, 2, 3, 3, 3, 1, 1]
    assert stats[0]["n_merged_components"] == 2
    reads = dict(given.merged_reads(problem))
    assert sorted(reads) == [0, 2, 5, 6]
    assert [v[0] for v in reads[0]] == list(range(0, 28)) and [v[0] for v in reads[2]] == list(range(20, 58))
    assert reads[5] == [tuple(v) for v in data["reads"][5]]
    # all alone: nothing is merged, every read passes through
    alone = rm.merge_batch([problem.with_representative(list(range(7)))], host=True)[0]
    assert int(alone.super_ptr[-1]) == 0 and [k for k, _ in alone.merged_reads(problem)] == list(range(7))
    for bad in ([1, 1, 2, 3, 4, 5, 6], [0, 0, 1, 3, 4, 5, 6], [0, 1, 2, 3, 4, 5, 7]):
        with pytest.raises(ValueError, match="representative"):
            rm.merge_batch([problem.with_representative(bad)], host=True)


def problem_of(reads, thr_diff=5, thr_neg_diff=3, rate=0.25):
    ptr = np.cumsum([0] + [len(r) for r in reads])
    flat = [v for r in reads for v in r]
    return rm.MergeProblem(ptr, [v[0] for v in flat], [v[1] for v in flat], [v[2] for v in flat], thr_diff, thr_neg_diff, rate)


def test_mismatched_lengths():
    with pytest.raises(ValueError, match="mismatched lengths"):
        rm.MergeProblem([0, 2], [1, 2, 3], [0, 0, 0], [1, 1, 1], 5, 3, 0.25)
    with pytest.raises(ValueError, match="mismatched lengths"):
        rm.MergeProblem([0, 2], [1, 2], [0, 0], [1], 5, 3, 0.25)
    with pytest.raises(ValueError, match="mismatched lengths"):
        rm.MergeProblem([0, 2, 3], [1, 2, 3], [0, 0, 0], [1, 1, 1], 5, 3, 0.25, representative=[0])


def test_refusals():
    ok = [[(1, 0, 5), (2, 1, 5)], [(2, 1, 5), (3, 0, 5)]]
    rm.merge_batch([problem_of(ok)], host=True)
    with pytest.raises(ValueError, match="read 1 has no variants"):
        rm.merge_batch([problem_of([ok[0], [], ok[1]])], host=True)
    with pytest.raises(ValueError, match="read 1: allele 255 outside"):
        rm.merge_batch([problem_of([ok[0], [(2, 2, 5)]])], host=True)
    with pytest.raises(ValueError, match="problem 1: read 0 has no variants"):
        rm.merge_batch([problem_of(ok), problem_of([[]])], host=True)
    bad = problem_of(ok)
    bad.read_ptr = np.array([0, 3, 2], dtype=np.uint64)
    with pytest.raises(ValueError, match="read_ptr decreases at read 1"):
        rm.merge_batch([bad], host=True)
    # positions: beyond int64 in Python, of magnitude 2^62 or more in the library
    with pytest.raises(_native.SolverError) as e:
        problem_of([[(1 << 63, 0, 5)]])
    assert e.value.status == _native.WHAMD_ERR_UNSUPPORTED
    for position in (1 << 62, -(1 << 62) - 1):
        with pytest.raises(_native.SolverError, match="2\\^62") as e:
            rm.merge_batch([problem_of([[(position, 0, 5)]])], host=True)
        assert e.value.status == _native.WHAMD_ERR_UNSUPPORTED
    rm.merge_batch([problem_of([[((1 << 62) - 1, 0, 5)], [(-(1 << 62), 0, 5)]])], host=True)
    # quality sums that could leave int64
    big = (1 << 62)
    with pytest.raises(_native.SolverError, match="2\\^63 - 1") as e:
        rm.merge_batch([problem_of([[(1, 0, big), (2, 0, big)]])], host=True)
    assert e.value.status == _native.WHAMD_ERR_UNSUPPORTED
    with pytest.raises(_native.SolverError, match="2\\^63 - 1"):
        rm.merge_batch([problem_of([[(1, 0, -big), (2, 0, -big), (3, 0, 1)]])], host=True)
    res = rm.merge_batch([problem_of([[(1, 0, big), (2, 0, big - 1)], [(1, 1, 0), (2, 0, 0)]], thr_diff=0, thr_neg_diff=0, rate=0.5)], host=True)[0]
    assert res.quality.tolist() == [big, big - 1]


def test_thresholds_far_outside_the_counts_are_clamped_not_wrapped():
    reads = [[(k, 0, 1) for k in range(8)], [(k, 0, 1) for k in range(8)]]
    assert rm.merge_batch([problem_of(reads, thr_diff=-(10 ** 30), thr_neg_diff=-(10 ** 30))], host=True)[0].representative.tolist() == [0, 0]
    assert rm.merge_batch([problem_of(reads, thr_diff=10 ** 30, thr_neg_diff=3)], host=True)[0].representative.tolist() == [0, 1]
    assert rm.merge_batch([problem_of(reads, thr_diff=5, thr_neg_diff=10 ** 30)], host=True)[0].representative.tolist() == [0, 1]


def test_missing_networkx_is_an_error_that_says_so(monkeypatch):
    import builtins

    real = builtins.__import__

    def no_networkx(name, *a, **k):
        if name == "networkx":
            raise ImportError("No module named 'networkx'")
        return real(name, *a, **k)

    spec = SPECS["not_blue_cuts_a_component"]
    monkeypatch.setattr(builtins, "__import__", no_networkx)
    with pytest.raises(ImportError, match="not-blue edges.*networkx"):
        rm.ReadMerger(*rc.merger_args(spec), host=True).merge(rc.readset_of(rc.materialize(spec)))
    # the common path does not need it
    spec = SPECS["chain"]
    assert len(rm.ReadMerger(*rc.merger_args(spec), host=True).merge(rc.readset_of(rc.materialize(spec)))) == 1


def test_install_read_merger_rebinds_and_restores():
    import types

    from whatshap_amd import shim
    from whatshap_amd.core import ReadSet

    old = object()
    phase = types.SimpleNamespace(ReadMerger=old, ReadSet=ReadSet)
    previous = shim.install_read_merger(phase)
    assert phase.ReadMerger is not old and previous.bindings == {"ReadMerger": old}
    merger = phase.ReadMerger(0.15, 0.25, 1000000, 1000)
    assert isinstance(merger, rm.ReadMerger)
    previous.restore()
    assert phase.ReadMerger is old
    assert rm.DoNothingReadMerger().merge(old) is old
