"""CPU: the polyphase threading DP through the one-thread host twin of the debug library (host=True) against what the reference's
HaploThreader made of the same cases (tests/golden/haplothread_cases.json.gz, written by tests/golden/make_haplothread_golden.py).
Every check of haplothread_cases.check_case runs on every case: (A) the reported score is the reference's optimum bit for bit, (B) so is
the returned path's cost under the recurrence, (C) the path has the right shape and uses the position's clusters only, (D) smoothed
coverages and coverage costs are the reference's, (E) where ambiguous == 0 the path is the reference's, slot order included."""
import numpy as np
import pytest

import haplothread_cases as hc
from whatshap_amd import _native, polythread, shim

GOLDEN = hc.load_golden()
CASES = GOLDEN["cases"]
BY_NAME = {c["name"]: c for c in CASES}
HOST = dict(host=True)


def test_the_record_is_of_the_generated_cases():
    made = hc.all_cases()
    assert [c["name"] for c in made] == [c["name"] for c in CASES]
    for a, b in zip(made, CASES):
        assert all(a[k] == b[k] for k in a), a["name"]


@pytest.fixture(scope="module")
def results():
    return polythread.thread_batch([hc.problem_of(c) for c in CASES], **HOST)


@pytest.mark.parametrize("k", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_case_against_the_reference(results, k):
    hc.check_case(CASES[k], results[k])


def test_at_least_half_of_the_random_cases_of_every_ploidy_are_unambiguous(results):
    """The cap on (E): a path check that ties could hide behind is none."""
    for p in hc.PLOIDIES:
        mine = [k for k, c in enumerate(CASES) if c["name"].startswith(f"random_p{p}_")]
        assert len(mine) == hc.RANDOM_PER_PLOIDY[p]
        unique = sum(1 for k in mine if not results[k].ambiguous.any())
        assert 2 * unique >= len(mine), (p, unique, len(mine))


def test_the_shapes_are_what_their_names_say(results):
    by = {c["name"]: results[k] for k, c in enumerate(CASES)}
    kept = {}
    for c in CASES:
        if c["small"]:   # what the reference's own costs leave within 30 of each column's smallest
            columns = [np.asarray([float.fromhex(h) for h in position], dtype=np.float32) for position in c["all_costs"]]
            kept[c["name"]] = [int((col <= np.float32(30.0) + col.min()).sum()) for col in columns]
            assert by[c["name"]].stats["n_entries"] == sum(kept[c["name"]]) and by[c["name"]].stats["n_tuples"] == sum(map(len, columns)), c["name"]
    assert kept["all_but_one_pruned"] == [1, 1, 1] and by["all_but_one_pruned"].stats["n_tuples"] == 9
    assert kept["none_pruned"] == [6, 6, 6] and by["none_pruned"].stats["n_tuples"] == 18       # a column of which nothing is pruned
    assert by["full_6_8"].stats["n_tuples"] == 3 * 1716 + 1 and by["full_5_7"].stats["n_tuples"] == 3 * 462 + 1
    assert by["full_6_8_shallow"].stats["n_entries"] > 3 * 1024                            # columns of more entries than a workgroup has lanes
    assert by["sections"].section_first.tolist() == [0, 1, 3, 4, 8]
    assert by["long_section"].score[0] > 2.0 ** 14                                         # the scores outgrew the float spacing of the costs
    assert any(r.ambiguous.any() for k, r in enumerate(results) if CASES[k]["tie_heavy"])
    assert all(r.stats["launches"] == 0 for r in results)                                  # the twin launches nothing


def test_a_batch_equals_the_calls_one_by_one(results):
    picked = [k for k, c in enumerate(CASES) if c["name"] in ("random_p2_s2000", "full_6_8", "sections", "random_p5_s5003", "one_position", "gap_0", "random_p4_s4001")]
    assert len(picked) == 7
    for k in picked:
        alone = polythread.thread_batch([hc.problem_of(CASES[k])], **HOST)[0]
        assert alone.tobytes() == results[k].tobytes(), CASES[k]["name"]


def test_compute_threading_path_has_the_references_signature(results):
    for name in ("random_p3_s3000", "readded_empty_rows", "disjoint_columns"):
        c = BY_NAME[name]
        cov_map, allele_depths = hc.dicts_of(c)
        got = polythread.compute_threading_path(cov_map, allele_depths, c["ploidy"], c["switch_cost"], c["affine_switch_cost"], c["max_gap"], **HOST)
        assert got == results[CASES.index(c)].paths.tolist() == c["path"]
    assert polythread.compute_threading_path([], [], 3, **HOST) == []


# ---------------------------------------------------------------------------------------------- refusals
def refused(match, exception=ValueError, **changes):
    c = dict(BY_NAME["random_p3_s3000"], **{k: v for k, v in changes.items() if k in BY_NAME["random_p3_s3000"]})
    extra = {k: v for k, v in changes.items() if k not in c}
    with pytest.raises(exception, match=match):
        polythread.thread_batch([hc.problem_of(c, **extra)], **HOST)


def test_refusals_name_their_limit():
    refused("ploidy 1 outside 2 .. 6", ploidy=1)
    refused("ploidy 7 outside 2 .. 6", ploidy=7)
    refused("row_limit 64: only 0", row_limit=64)
    refused("not exact in float", switch_cost=0.1, affine_switch_cost=0.1)
    refused("multiples of 2\\^-20", switch_cost=2.0 ** -30, affine_switch_cost=0.0)
    refused("not negative", switch_cost=-1.0)
    refused("not negative", affine_switch_cost=float("nan"))
    refused("not negative", switch_cost=float("inf"))
    c = BY_NAME["random_p3_s3000"]
    refused("position 2: its cov_map row is empty", cov_map=c["cov_map"][:2] + [[]] + c["cov_map"][3:])
    refused("position 1 lists cluster", cov_map=[c["cov_map"][0], c["cov_map"][1] + c["cov_map"][1][:1]] + c["cov_map"][2:])
    nine = list(range(100, 109))
    with pytest.raises(_native.SolverError, match="position 0 lists 9 clusters: more than 8") as e:
        polythread.thread_batch([hc.problem_of(hc.case("nine", 2, [nine], [[[g, 5] for g in nine]]))], **HOST)
    assert e.value.status == _native.WHAMD_ERR_UNSUPPORTED
    refused("has no depth row", IndexError, depths=[c["depths"][0], [r for r in c["depths"][1] if r[0] != c["cov_map"][1][0]]] + c["depths"][2:])
    refused("block_starts must begin with 0", block_starts=[1])
    refused("block_starts must begin with 0", block_starts=[0, 5, 3])
    refused("block_starts is empty", block_starts=[])
    with pytest.raises(IndexError):
        polythread.compute_threading_path([[1, 2]], [{1: {0: 3}}], 2, **HOST)


def test_the_pipelines_integer_costs_always_pass():
    for affine in (1, 2, 3, 7, 50, 1000, 65536):
        c = dict(BY_NAME["two_positions"], switch_cost=4.0 * affine, affine_switch_cost=float(affine))
        polythread.thread_batch([hc.problem_of(c)], **HOST)


# ---------------------------------------------------------------------------------------------- the pipeline, the shim
def test_run_threading_end_to_end_against_the_chain_of_recorded_pieces():
    import polythread_cases as pc

    recorded = pc.load_golden()["cases"]
    seen = 0
    for rec in GOLDEN["pipeline"]:
        case = recorded[rec["index"]]
        assert case["name"] == rec["name"] and case["cov_map"] == rec["cov_map"]
        matrix = pc.problem_of(case).matrix
        calls = []

        def force(paths, haplotypes, genotypes, cov_map, allele_depths, error_rate):
            calls.append((cov_map, [{cid: dict(d) for cid, d in position.items()} for position in allele_depths], error_rate))
            return haplotypes

        paths, haplotypes = polythread.run_threading(matrix, case["clustering"], case["ploidy"], [{} for _ in range(case["n_pos"])], False, case["max_gap"], 0.07,
                                                     force_genotypes=force, **HOST)
        # the threader's piece: the recorded inputs through the reference's signature, and the reference's own path where it is defined
        cov_map, allele_depths = case["cov_map"], [{cid: dict(map(tuple, alleles)) for cid, alleles in position} for position in case["ad_after"]]
        assert paths == polythread.compute_threading_path(cov_map, allele_depths, case["ploidy"], rec["switch_cost"], rec["affine_switch_cost"], case["max_gap"], **HOST)
        res = polythread.thread_batch([hc.problem_of(rec)], **HOST)[0]
        hc.check_case(rec, res)
        assert paths == res.paths.tolist()
        # the haplotypes' piece
        cons = [{cid: picks for cid, picks in position} for position in case["cons_lists"]]
        assert haplotypes == polythread.compute_haplotypes(paths, cons, case["ploidy"], **HOST)
        assert calls == [(cov_map, allele_depths, 0.07)]
        seen += 1
        with pytest.raises(ValueError, match="pass force_genotypes"):
            polythread.run_threading(matrix, case["clustering"], case["ploidy"], [], False, case["max_gap"], **HOST)
        again = polythread.run_threading(matrix, case["clustering"], case["ploidy"], [], True, case["max_gap"], **HOST)
        assert again == (paths, haplotypes)
    assert seen >= 20


def test_install_threading_rebinds_compute_threading_path_only(monkeypatch):
    import types

    module = types.SimpleNamespace(compute_threading_path=lambda *a, **k: "reference", select_clusters="kept", force_genotypes="kept")
    seen = {}

    def fake(cov_map, allele_depths, ploidy, switch_cost, affine_switch_cost, max_cluster_gap, *, device=0, host=False):
        seen.update(device=device, costs=(switch_cost, affine_switch_cost, max_cluster_gap))
        return polythread_compute(cov_map, allele_depths, ploidy, switch_cost, affine_switch_cost, max_cluster_gap, host=True)

    polythread_compute = polythread.compute_threading_path
    monkeypatch.setattr(polythread, "compute_threading_path", fake)
    previous = shim.install_threading(module, device=3)
    c = BY_NAME["disjoint_columns"]
    cov_map, allele_depths = hc.dicts_of(c)
    assert module.compute_threading_path(cov_map, allele_depths, c["ploidy"], switch_cost=12.0, affine_switch_cost=3.0, max_cluster_gap=10) == c["path"]
    assert seen == {"device": 3, "costs": (12.0, 3.0, 10)}
    assert module.select_clusters == "kept" and module.force_genotypes == "kept"
    assert list(previous.bindings) == ["compute_threading_path"]
    previous.restore()
    assert module.compute_threading_path() == "reference"
