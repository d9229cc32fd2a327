"""GPU: the polyphase threading inputs on the device (csrc/polythread_device.hip) against everything the reference recorded in
tests/golden/polythread_cases.json.gz, and byte for byte against the host twin on seeded larger shapes the fixture cannot hold: a run
of several thousand entries next to runs of one (every run class), positions on both sides of the scan tiles' ends, 200 blocks in one
call.  The launch count does not depend on the batch."""
import numpy as np
import pytest

import polythread_cases as pc
from whatshap_amd import _native
from whatshap_amd import polythread as pt

pytestmark = pytest.mark.gpu

GOLDEN = pc.load_golden()
CASES = GOLDEN["cases"]


@pytest.fixture(scope="module")
def device_results():
    stats = []
    return pt.threading_inputs_batch([pc.problem_of(c) for c in CASES], stats=stats), stats


def same_bytes(problems):
    stats = []
    got = pt.threading_inputs_batch(problems, stats=stats)
    want = pt.threading_inputs_batch(problems, host=True)
    for k, (g, w) in enumerate(zip(got, want)):
        for name in pt.ThreadingInputs.ARRAYS:
            assert np.array_equal(getattr(g, name), getattr(w, name)), (k, name)
        assert g.tobytes() == w.tobytes()
        for key in ("n_rows", "n_selected", "n_readded", "n_emptied", "positions_class_a", "positions_class_b", "positions_class_c"):
            assert g.stats[key] == w.stats[key], (k, key)
    return got, stats


def test_device_equals_every_recorded_case(device_results):
    results, stats = device_results
    for res, rec in zip(results, CASES):
        pc.check_against_record(res, rec)
    assert all(s["launches"] == _native.POLY_THREAD_LAUNCHES for s in stats)


def test_device_equals_the_host_twin_on_the_recorded_cases(device_results):
    want = pt.threading_inputs_batch([pc.problem_of(c) for c in CASES], host=True)
    for g, w, rec in zip(device_results[0], want, CASES):
        assert g.tobytes() == w.tobytes(), rec["name"]


def test_reference_signature_functions_on_the_device():
    for rec in CASES[:12] + [GOLDEN["uncovered"]]:
        ad, cons = pt.get_allele_depths(pc.matrix_of(rec), rec["clustering"], rec["ploidy"])
        assert pc.as_pairs(ad) == rec["ad"] and pc.as_pairs(cons) == rec["cons_lists"], rec["name"]
    for rec in [c for c in CASES if not c["name"].startswith("random")] + CASES[-2:]:
        ad = pc.as_dicts(rec["ad"])
        assert pt.select_clusters(ad, rec["ploidy"], rec["max_gap"]) == rec["cov_map"], rec["name"]
        assert pc.as_pairs(ad) == rec["ad_after"], rec["name"]
        cons = [{cid: picks for cid, picks in position} for position in rec["cons_lists"]]
        for paths, want in zip(rec["paths"], rec["haplotypes"]):
            assert pt.compute_haplotypes(paths, cons, rec["ploidy"]) == want, rec["name"]
    for rec in GOLDEN["select"]:
        ad = pc.as_dicts(rec["depths"])
        assert pt.select_clusters(ad, rec["ploidy"], rec["max_gap"]) == rec["cov_map"], rec["name"]
        assert pc.as_pairs(ad) == rec["ad_after"], rec["name"]
    assert pt.compute_haplotypes([[0, 0, 7]], [{0: [1, 0, 1]}], 3) == [[1], [0], [-1]]


def test_haplotypes_from_the_arrays(device_results):
    for res, rec in zip(device_results[0], CASES):
        for paths, want in zip(rec["paths"], rec["haplotypes"]):
            assert pt.haplotypes_from_inputs(paths, res).tolist() == want, rec["name"]


def test_every_run_class_in_one_problem():
    """A position of 6 000 entries over five clusters (one workgroup), one of 300 (one wave), positions of one or two (eight lanes)."""
    got, stats = same_bytes([pc.problem_of(pc.long_run_case())])
    s = stats[0]
    assert s["positions_class_c"] == 1 and s["positions_class_b"] == 2 and s["positions_class_a"] == 9
    assert int(got[0].pc_depth.sum()) <= s["n_counted"] and s["n_rows"] == len(got[0].pc_cluster)   # (emptied rows count no more)


def test_positions_on_both_sides_of_the_scan_tiles():
    """2 * 2048 + 1 positions: entries left and right of every scan tile's end, in the run offsets and in the row offsets."""
    arrays = pc.array_problem(21, 2 * 2048 + 1, 12, 4, 3, 9, 3, max_gap=5)
    got, stats = same_bytes([pc.problem_of_arrays(arrays, 4, 5)])
    assert stats[0]["n_positions"] == 2 * 2048 + 1 and stats[0]["n_readded"] > 0
    ptr = got[0].pc_ptr
    assert all(ptr[x + 1] > ptr[x] for x in (2047, 2048, 4095, 4096))


def test_sixteen_alleles_and_ploidy_sixteen():
    arrays = pc.array_problem(22, 300, 40, 16, 16, 6, 2, max_gap=3)
    same_bytes([pc.problem_of_arrays(arrays, 16, 3), pc.problem_of_arrays(pc.array_problem(23, 50, 9, 2, 2, 5, 1), 2, 0)])


def test_sixteen_alleles_in_one_wave_and_in_one_workgroup():
    """The sixteen-allele rows of class b (one wave) and class c (one workgroup): a position of 300 entries and one of 4 200, each over
    four clusters and all sixteen alleles, ploidy 16, next to positions of one entry."""
    got, stats = same_bytes([pc.problem_of(pc.sixteen_allele_long_runs_case())])
    s = stats[0]
    assert s["positions_class_b"] >= 1 and s["positions_class_c"] >= 1 and s["positions_class_a"] == 5
    assert got[0].n_alleles == 16 and got[0].pc_depth.shape[1] == 16   # (more than four alleles: the rows keep NA = 16)
    assert s["n_counted"] == 4200 + 300 + 5 and int(got[0].pc_depth.sum()) <= s["n_counted"]   # (emptied rows count no more)


@pytest.mark.parametrize("n_entries", [1, 256, 257, 600])
def test_reads_at_a_workgroup_edge(n_entries):
    """The read lookup of the count and place launches where a workgroup's 256 entries end: single-entry reads at entries 255 and 256
    with empty reads before, between and behind them (polythread_cases.EDGE_READ_LENGTHS), and the same reads cut to 1, 256 and 257
    entries.  AlleleMatrix.from_csr takes reads without entries as they are."""
    arrays = pc.edge_reads_arrays(n_entries)
    assert np.diff(arrays[0].astype(np.int64)).tolist() == np.diff(np.minimum(np.cumsum((0,) + pc.EDGE_READ_LENGTHS), n_entries)).tolist()
    got, stats = same_bytes([pc.problem_of_arrays(arrays, 2, 3)])
    assert stats[0]["n_entries"] == stats[0]["n_counted"] == n_entries and stats[0]["n_reads"] == len(pc.EDGE_READ_LENGTHS)


def test_a_batch_of_200_blocks_and_the_launch_count():
    blocks = [pc.problem_of_arrays(arrays, ploidy, gap) for arrays, ploidy, gap in pc.small_blocks(200)]
    got, stats = same_bytes(blocks)
    assert len(got) == 200 and {s["launches"] for s in stats} == {_native.POLY_THREAD_LAUNCHES}
    one = []
    alone = pt.threading_inputs_batch(blocks[:1], stats=one)[0]
    assert one[0]["launches"] == stats[0]["launches"] == _native.POLY_THREAD_LAUNCHES
    assert alone.tobytes() == got[0].tobytes()
    for k in (1, 57, 199):
        assert pt.threading_inputs_batch([blocks[k]])[0].tobytes() == got[k].tobytes()


def test_refusals_launch_nothing():
    rec = GOLDEN["uncovered"]
    with pytest.raises(ValueError, match="position 2 has no counted entry"):
        pt.threading_inputs_batch([pc.problem_of(rec)])
    with pytest.raises(IndexError):
        pt.threading_inputs(pc.matrix_of(rec), rec["clustering"], rec["ploidy"], rec["max_gap"])
    with pytest.raises(ValueError, match="is in two clusters"):
        pt.threading_inputs_batch([pt.ThreadingProblem(pc.matrix_of(CASES[0]), [[0, 1], [1]], 2)])
    with pytest.raises(ValueError, match="ploidy 17"):
        pt.threading_inputs_batch([pt.ThreadingProblem(pc.matrix_of(CASES[0]), CASES[0]["clustering"], 17)])
    with pytest.raises(ValueError, match="allele 1 outside"):
        pt.threading_inputs_batch([pt.ThreadingProblem(pc.matrix_of(CASES[5]), CASES[5]["clustering"], 2, n_alleles=1)])
