"""GPU: the polyphase threading inputs on the device (csrc/polythread_device.hip) against everything the reference recorded in
tests/golden/polythread_cases.json.gz, and byte for byte against the host twin on seeded larger shapes the fixture cannot hold: a run
of several thousand entries next to runs of one (every run class), positions on both sides of the scan tiles' ends, 200 blocks in one
call.  The launch count does not depend on the batch.  Where the teams, the scans and the three shared functions change path -- every
class boundary, a cluster per entry, 257 scan tiles, consensus ties at depth, the selection's exact threshold, the haplotype kernel's
second workgroup -- the device is also held to polythread_cases' plain restatement, which shares no code with the library."""
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


# ---------------------------------------------------------------------------------------------- against the plain restatement
# The shapes at which the shared transposition, the teams and the scans change path, each compared with polythread_cases' restatement
# (rows, depths, first, consensus lists, own selection: no code shared with the library) and byte for byte with the host twin.
K = pc.header_constants()
RUNS = pc.boundary_runs(K)


def device_and_restatement(blocks):
    """(arrays, ploidy, max_gap) blocks in one call: (results, stats, restated rows)."""
    got, stats = same_bytes([pc.problem_of_arrays(*b) for b in blocks])
    assert {s["launches"] for s in stats} == {_native.POLY_THREAD_LAUNCHES}
    return got, stats, [pc.check_against_restatement(g, arrays, ploidy) for g, (arrays, ploidy, _) in zip(got, blocks)]


def test_the_run_lengths_are_those_around_the_headers_constants():
    assert (K["RS_SEGMENT"], K["WAVE"], K["RS_BLOCK"], K["PT_CLASS_A_MAX"], K["PT_CLASS_B_MAX"], K["RS_SCAN_TILE"]) == (8, 64, 256, 64, 4096, 2048)
    assert RUNS == (1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4095, 4096, 4097)
    assert pc.classes_of(RUNS, K["PT_CLASS_A_MAX"], K["PT_CLASS_B_MAX"]) == (7, 9, 1)


@pytest.mark.parametrize("k, n_rows", [(1, 17), (3, 48), (9, 135)])
@pytest.mark.parametrize("n_alleles, ploidy", [(3, 3), (16, 16)])
def test_every_class_boundary(n_alleles, ploidy, k, n_rows):
    """Runs of the segment's, the wave's and the workgroup's width and of both class bounds, each and its two neighbours, over
    min(k, run) clusters -- nine is more than a segment has lanes --, with four and with sixteen alleles per row."""
    got, stats, want = device_and_restatement([pc.boundary_problem(RUNS, k, ploidy, n_alleles)])
    s = stats[0]
    assert (s["positions_class_a"], s["positions_class_b"], s["positions_class_c"]) == pc.classes_of(RUNS, K["PT_CLASS_A_MAX"], K["PT_CLASS_B_MAX"]) == (7, 9, 1)
    assert s["n_rows"] == len(want[0].cluster) == n_rows == sum(min(k, r) for r in RUNS)
    assert got[0].n_alleles == n_alleles and s["n_counted"] == sum(RUNS)


def test_as_many_clusters_as_entries():
    """Every entry in a cluster of its own: the walk makes one trip per entry in each class, the ordinal runs past 4 096 in the
    workgroup class, every row has total 1."""
    runs = (K["PT_CLASS_B_MAX"] + 1, K["PT_CLASS_A_MAX"] + 1, 1)
    got, stats, want = device_and_restatement([pc.runs_problem(runs, runs, 2, 2, seed=4163)])
    s = stats[0]
    assert (s["positions_class_a"], s["positions_class_b"], s["positions_class_c"]) == (1, 1, 1)
    assert s["n_rows"] == len(want[0].cluster) == sum(runs) == 4163 and (want[0].total == 1).all()
    assert np.diff(got[0].pc_ptr.astype(np.int64)).tolist() == list(runs)


def test_both_scans_across_the_carry():
    """257 scan tiles, one more than the second scan launch's workgroup takes per pass: the class b and the class c run lie in the
    last full tile, so their placed slots and their rows begin behind the carry; the row scan's total sizes the result image."""
    blocks = [pc.carry_problem(K["RS_SCAN_TILE"])]
    got, stats, want = device_and_restatement(blocks)
    s, ptr = stats[0], got[0].pc_ptr.astype(np.int64)
    assert s["n_positions"] == K["RS_SCAN_TILE"] * K["RS_BLOCK"] + 1 == 524_289
    assert (s["positions_class_a"], s["positions_class_b"], s["positions_class_c"]) == (524_287, 1, 1)
    assert s["n_rows"] == len(got[0].pc_cluster) == len(want[0].cluster) == 524_310
    for x, (run, clusters) in pc.CARRY_KEYS.items():
        assert ptr[x + 1] - ptr[x] == clusters and want[0].total[ptr[x]:ptr[x + 1]].sum() == run, x


@pytest.mark.parametrize("alleles, n_alleles", [((0, 1), 2), ((14, 15), 16)])
def test_consensus_ties_at_depth_in_the_wave_and_workgroup_classes(alleles, n_alleles):
    """Depths 3000 : 1500 in one workgroup and 200 : 100 in one wave, ploidy 4: the second pick is a tie and goes to the allele a read
    of the cluster's list shows first -- once a read of the one, once of the other, and the two lists differ."""
    cases = pc.tie_cases(alleles, n_alleles)
    got, stats = same_bytes([pc.problem_of(c) for c in cases])
    pc.check_ties(got, cases, alleles)
    for s in stats:
        assert (s["positions_class_b"], s["positions_class_c"], s["launches"]) == (1, 1, _native.POLY_THREAD_LAUNCHES)
    assert got[0].n_alleles == n_alleles


def test_selection_at_the_exact_threshold_on_the_device():
    """select_clusters on the device: 336 positions a call (a second workgroup of the stand-alone select launch), every ploidy."""
    pc.check_exact_thresholds(lambda depths, ploidy: pt.select_clusters(depths, ploidy, 0))


@pytest.mark.parametrize("ploidy", [2, 6, 16])
def test_the_haplotype_kernel_past_one_workgroup(ploidy):
    """haplotypes_from_inputs at 255, 256, 257 and 2 049 positions on seeded paths: clusters named twice, clusters without a row."""
    blocks = pc.haplotype_blocks(ploidy)
    got, _, _ = device_and_restatement(blocks)

    def run(paths, res):
        out = pt.haplotypes_from_inputs(paths, res)
        assert np.array_equal(out, pt.haplotypes_from_inputs(paths, res, host=True))
        return out

    pc.check_haplotypes(got, blocks, run)
    assert [len(g.pc_ptr) - 1 for g in got] == list(pc.HAPLOTYPE_POSITIONS)


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
