"""CPU: the host twin of the polyphase threading inputs (debug library, one thread; the kernels call the same consensus, selection and
haplotype functions) against everything the reference recorded in tests/golden/polythread_cases.json.gz -- arrays, dict forms, insertion
orders, the mutation select_clusters leaves --, the refusals, and the reference-signature functions.  polythread_cases' plain
restatement is held to the same record, and the twin to the restatement on the shapes the GPU tests run."""
import copy

import numpy as np
import pytest

import polythread_cases as pc
from whatshap_amd import _native
from whatshap_amd import polythread as pt
from whatshap_amd.polyphase import AlleleMatrix

GOLDEN = pc.load_golden()
CASES = GOLDEN["cases"]


@pytest.fixture(scope="module")
def host_results():
    return pt.threading_inputs_batch([pc.problem_of(c) for c in CASES], host=True)


def test_the_fixture_is_what_the_generator_would_record():
    """The recorded inputs are the seeded generator's of today: no case was dropped or edited by hand."""
    made = pc.all_cases()
    assert [c["name"] for c in made] == [c["name"] for c in CASES] and len(CASES) >= 36
    for a, b in zip(made, CASES):
        assert all(a[k] == b[k] for k in a)
    assert [c["name"] for c in pc.select_cases()] == [c["name"] for c in GOLDEN["select"]]
    assert GOLDEN["emptied_rows"] >= 1
    assert {c["ploidy"] for c in CASES} >= {1, 2, 3, 4, 6}
    assert {1 + max(a for r in c["reads"] for _, a in r) for c in CASES} >= {2, 3, 4}


def test_host_twin_equals_every_recorded_case(host_results):
    for res, rec in zip(host_results, CASES):
        pc.check_against_record(res, rec)
        assert res.stats["launches"] == 0


def test_a_batch_equals_the_problems_one_by_one(host_results):
    for res, rec in zip(host_results, CASES[:24]):
        alone = pt.threading_inputs_batch([pc.problem_of(rec)], host=True)[0]
        assert alone.tobytes() == res.tobytes(), rec["name"]


def test_positions_far_apart_give_the_same_rows(host_results):
    """The matrix builder ranks positions through a bitmap of their span where that is small and through a sort where it is not: the
    same cases with 50 000 000 between neighbouring positions (the sort) give the bytes of the compact ones (the bitmap)."""
    picked = [k for k, c in enumerate(CASES) if c["n_pos"] <= 60][:30]
    spread = []
    for k in picked:
        c = CASES[k]
        read_ptr, pos, alle = pc.csr_of(c)
        am = AlleleMatrix.from_csr(read_ptr, (pos - 100) // 7 * 50_000_000 + 5, alle)
        spread.append(pt.ThreadingProblem(am, c["clustering"], c["ploidy"], c["max_gap"]))
    for k, res in zip(picked, pt.threading_inputs_batch(spread, host=True)):
        assert res.tobytes() == host_results[k].tobytes(), CASES[k]["name"]
        assert spread[picked.index(k)].matrix.getNumPositions() == CASES[k]["n_pos"]


def test_switch_costs(host_results):
    from math import ceil

    for res, rec in zip(host_results, CASES):
        ratio = float.fromhex(rec["ratio"])
        assert pt.compute_readlength_snp_distance_ratio(pc.matrix_of(rec)) == ratio
        assert res.affine_switch_cost == ceil(ratio / 1.0) and res.switch_cost == 4 * ceil(ratio / 1.0)


def test_get_allele_depths_in_the_reference_order():
    for rec in CASES + [GOLDEN["uncovered"]]:
        ad, cons = pt.get_allele_depths(pc.matrix_of(rec), rec["clustering"], rec["ploidy"], host=True)
        assert pc.as_pairs(ad) == rec["ad"], rec["name"]
        assert pc.as_pairs(cons) == rec["cons_lists"], rec["name"]


def test_select_clusters_leaves_its_argument_as_the_reference_does():
    for rec in CASES:
        ad = pc.as_dicts(rec["ad"])
        assert pt.select_clusters(ad, rec["ploidy"], rec["max_gap"], host=True) == rec["cov_map"], rec["name"]
        assert pc.as_pairs(ad) == rec["ad_after"], rec["name"]
    for rec in GOLDEN["select"]:
        ad = pc.as_dicts(rec["depths"])
        assert pt.select_clusters(ad, rec["ploidy"], rec["max_gap"], host=True) == rec["cov_map"], rec["name"]
        assert pc.as_pairs(ad) == rec["ad_after"], rec["name"]


def test_a_position_without_a_counted_entry():
    rec = GOLDEN["uncovered"]
    assert rec["raises"] == "IndexError"
    with pytest.raises(ValueError, match="position 2 has no counted entry"):
        pt.threading_inputs_batch([pc.problem_of(rec)], host=True)
    with pytest.raises(IndexError):
        pt.threading_inputs(pc.matrix_of(rec), rec["clustering"], rec["ploidy"], rec["max_gap"], host=True)
    ad = pc.as_dicts(rec["ad"])
    before = copy.deepcopy(ad)
    with pytest.raises(IndexError):
        pt.select_clusters(ad, rec["ploidy"], rec["max_gap"], host=True)
    assert ad == before


def test_compute_haplotypes():
    for rec in CASES:
        cons = [{cid: picks for cid, picks in position} for position in rec["cons_lists"]]
        for paths, want in zip(rec["paths"], rec["haplotypes"]):
            before = copy.deepcopy((paths, cons))
            assert pt.compute_haplotypes(paths, cons, rec["ploidy"], host=True) == want, rec["name"]
            assert (paths, cons) == before
    assert pt.compute_haplotypes([[0, 0, 7]], [{0: [1, 0, 1]}], 3, host=True) == [[1], [0], [-1]]
    with pytest.raises(IndexError):   # a list shorter than the slots that ask for it, as the reference's indexing raises
        pt.compute_haplotypes([[0, 0]], [{0: [1]}], 2, host=True)
    assert pt.compute_haplotypes([[0, 1]], [{0: [1], 1: [0, 0]}], 2, host=True) == [[1], [0]]


def test_haplotypes_from_the_arrays(host_results):
    for res, rec in zip(host_results, CASES):
        for paths, want in zip(rec["paths"], rec["haplotypes"]):
            assert pt.haplotypes_from_inputs(paths, res, host=True).tolist() == want, rec["name"]


def test_threading_inputs_gives_the_shapes_the_threader_takes():
    rec = next(c for c in CASES if c["name"] == "readded_without_a_row_next_to_an_emptied_one")
    got = pt.threading_inputs(pc.matrix_of(rec), rec["clustering"], rec["ploidy"], rec["max_gap"], host=True)
    assert got["cov_map"] == rec["cov_map"] and pc.as_pairs(got["allele_depths"]) == rec["ad_after"] and pc.as_pairs(got["cons_lists"]) == rec["cons_lists"]
    assert got["switch_cost"] == 4 * got["affine_switch_cost"] == 4
    for x, clusters in enumerate(got["cov_map"]):   # what computePathsBlockwise indexes
        assert all(cid in got["allele_depths"][x] for cid in clusters)


def tiny(reads=(((0, 0), (1, 1)), ((0, 1), (1, 0))), clustering=((0,), (1,)), ploidy=2, **kw):
    read_ptr = np.cumsum([0] + [len(r) for r in reads])
    am = AlleleMatrix.from_csr(read_ptr, [pc.global_position(p) for r in reads for p, _ in r], [a for r in reads for _, a in r])
    return pt.ThreadingProblem(am, [list(c) for c in clustering], ploidy, **kw)


@pytest.mark.parametrize("problem, message", [
    (dict(clustering=((0, 1), (1,))), "read 1 is in two clusters"),
    (dict(clustering=((0, 0), (1,))), "read 0 is in two clusters"),
    (dict(clustering=((0,), (2,))), "read id 2 out of range"),
    (dict(n_alleles=1), "allele 1 outside 0 .. 0"),
    (dict(n_alleles=17), "n_alleles 17 outside 1 .. 16"),
    (dict(ploidy=17), "ploidy 17 outside 1 .. 16"),
    (dict(ploidy=0), "ploidy 0 outside 1 .. 16"),
    (dict(reads=(((0, 0), (1, 1)), ((1, 1), (2, 0))), clustering=((0,),)), "position 2 has no counted entry"),
])
def test_refusals(problem, message):
    with pytest.raises(ValueError, match=message):
        pt.threading_inputs_batch([tiny(**problem)], host=True)
    with pytest.raises(ValueError, match="problem 1: .*" + message):   # in a batch the message names the problem
        pt.threading_inputs_batch([tiny(), tiny(**problem)], host=True)


def test_refusals_of_the_array_calls():
    with pytest.raises(ValueError, match="ploidy 17"):
        pt.select_clusters([{0: {0: 1}}], 17, 1, host=True)
    with pytest.raises(ValueError, match="ploidy 17"):
        pt.compute_haplotypes([[0] * 17], [{0: [0] * 17}], 17, host=True)
    with pytest.raises(ZeroDivisionError):
        pt.select_clusters([{0: {}, 1: {}}], 2, 1, host=True)
    assert pt.select_clusters([{3: {}}], 2, 1, host=True) == [[3]]


def test_larger_ploidy_and_allele_counts_up_to_the_bounds():
    """Ploidy 16 and 16 alleles: the instantiation with sixteen alleles per row, against a plain restatement of the two loops."""
    rng = np.random.default_rng(3)
    reads = [[(p, int(rng.integers(0, 16))) for p in range(4)] for _ in range(60)]
    clustering = [list(range(0, 60, 3))[::-1], list(range(1, 60, 3)), list(range(2, 60, 3))]
    res = pt.threading_inputs_batch([tiny(reads=reads, clustering=clustering, ploidy=16, n_alleles=16)], host=True)[0]
    ad, cons = res._dicts()
    for x in range(4):
        for cid, members in enumerate(clustering):
            want = {}
            for r in members:
                want[reads[r][x][1]] = want.get(reads[r][x][1], 0) + 1
            assert list(ad[x][cid].items()) == list(want.items())
            picks, cnts = [], {}
            for _ in range(16):
                best, best_al = 0, 0
                for al, n in want.items():
                    q = n / (1 + cnts.get(al, 0))
                    if q > best:
                        best, best_al = q, al
                picks.append(best_al)
                cnts[best_al] = cnts.get(best_al, 0) + 1
            assert cons[x][cid] == picks


# ---------------------------------------------------------------------------------------------- the plain restatement
def recorded_rows(rec, n_alleles):
    """(ptr, cluster, depth rows, allele orders, consensus lists) of a recorded case, before select_clusters' side effect."""
    ptr, cluster, depth, order, cons = [0], [], [], [], []
    for before, lists in zip(rec["ad"], rec["cons_lists"]):
        lists = dict((cid, picks) for cid, picks in lists)
        for cid, alleles in sorted(before):
            row = [0] * n_alleles
            for a, n in alleles:
                row[a] = n
            cluster.append(cid)
            depth.append(row)
            order.append([a for a, _ in alleles])
            cons.append(lists[cid])
        ptr.append(len(cluster))
    return ptr, cluster, depth, order, cons


def test_the_restatement_equals_every_recorded_case():
    """polythread_cases' numpy / Python restatement, which shares nothing with the library, against the reference's record: rows,
    depths before the side effect, insertion orders, consensus lists, each position's own selection and the haplotypes."""
    for rec in CASES + [GOLDEN["uncovered"]]:
        n_alleles = max([a for r in rec["reads"] for _, a in r], default=0) + 1
        rows = pc.restate_rows(*pc.csr_of(rec), rec["clustering"], n_alleles)
        ptr, cluster, depth, order, cons = recorded_rows(rec, n_alleles)
        assert rows.n_pos == rec["n_pos"] and rows.ptr.tolist() == ptr and rows.cluster.tolist() == cluster, rec["name"]
        assert rows.depth.tolist() == depth and rows.total.tolist() == [sum(row) for row in depth], rec["name"]
        for first, shown, alleles in zip(rows.first.tolist(), depth, order):
            assert [first[a] == pc.NO_READ for a in range(n_alleles)] == [n == 0 for n in shown], rec["name"]
            assert sorted((a for a in range(n_alleles) if shown[a]), key=lambda a: first[a]) == alleles, rec["name"]
        assert [pc.restate_consensus(d, f, rec["ploidy"]) for d, f in zip(rows.depth.tolist(), rows.first.tolist())] == cons, rec["name"]
        consensus = pc.restate_consensus_rows(rows.depth, rows.first, rec["ploidy"])
        assert consensus.tolist() == cons, rec["name"]
        if "cov_map" not in rec:   # (the refused case: the reference's select_clusters raises)
            continue
        sel_ptr, sel_row = pc.restate_selections(rows.ptr, rows.total, rec["ploidy"])
        for x, (before, after, listed) in enumerate(zip(rec["ad"], rec["ad_after"], rec["cov_map"])):
            own = rows.cluster[sel_row[sel_ptr[x]:sel_ptr[x + 1]]].tolist()
            assert sel_row[sel_ptr[x]:sel_ptr[x + 1]].tolist() == [ptr[x] + k for k in pc.restate_selection(rows.total[ptr[x]:ptr[x + 1]].tolist(), rec["ploidy"])]
            # the recorded list is the own selection and what the gap filling re-added, which the record shows as an emptied or a new dict
            before = dict((cid, v) for cid, v in before)
            readded = {cid for cid, v in after if not v and before.get(cid) != v}
            assert sorted(own) == [cid for cid in listed if cid not in readded], (rec["name"], x)
            if rec["max_gap"] == 0 or x in (0, rec["n_pos"] - 1):   # (no gap filling there: the list is the own selection)
                assert sorted(own) == listed, (rec["name"], x)
        for paths, want in zip(rec["paths"], rec["haplotypes"]):
            assert pc.restate_haplotypes(paths, rows.ptr, rows.cluster, consensus, rec["ploidy"]).tolist() == want, rec["name"]
    assert pc.restate_haplotypes([[0, 0, 7]], [0, 1], [0], [[1, 0, 1]], 3).tolist() == [[1], [0], [-1]]
    assert sum(rec["max_gap"] == 0 for rec in CASES) >= 1


def test_the_restated_selection_equals_the_recorded_dict_level_cases():
    """GOLDEN["select"]: clusters in dict order, equal depths, empty inner dicts."""
    for rec in GOLDEN["select"]:
        n_pos = len(rec["depths"])
        for x, (before, after, listed) in enumerate(zip(rec["depths"], rec["ad_after"], rec["cov_map"])):
            own = [before[k][0] for k in pc.restate_selection([sum(n for _, n in alleles) for _, alleles in before], rec["ploidy"])]
            known = dict((cid, v) for cid, v in before)
            readded = {cid for cid, v in after if not v and known.get(cid) != v}
            assert sorted(own) == [cid for cid in listed if cid not in readded], (rec["name"], x)
            if x in (0, n_pos - 1):
                assert sorted(own) == listed, (rec["name"], x)


def host_and_restatement(blocks):
    """The host twin on (arrays, ploidy, max_gap) blocks, every result against the restatement of its input."""
    got = pt.threading_inputs_batch([pc.problem_of_arrays(*b) for b in blocks], host=True)
    return got, [pc.check_against_restatement(g, arrays, ploidy) for g, (arrays, ploidy, _) in zip(got, blocks)]


def test_host_twin_equals_the_restatement_on_the_recorded_cases(host_results):
    for res, rec in zip(host_results, CASES):
        pc.check_against_restatement(res, pc.arrays_of(rec), rec["ploidy"])


@pytest.mark.parametrize("n_alleles, ploidy", [(3, 3), (16, 16)])
def test_host_twin_equals_the_restatement_at_every_class_boundary(n_alleles, ploidy):
    runs = pc.boundary_runs()
    got, want = host_and_restatement([pc.boundary_problem(runs, k, ploidy, n_alleles) for k in (1, 3, 9)])
    assert [len(w.cluster) for w in want] == [17, 48, 135] == [g.stats["n_rows"] for g in got]
    assert all(g.n_alleles == n_alleles for g in got)


def test_host_twin_equals_the_restatement_across_257_scan_tiles_and_with_a_cluster_per_entry():
    got, want = host_and_restatement([pc.carry_problem(), pc.runs_problem((4097, 65, 1), (4097, 65, 1), 2, 2, seed=4163)])
    assert got[0].stats["n_rows"] == len(want[0].cluster) == 524_310 and got[0].stats["n_positions"] == 2048 * 256 + 1
    assert len(want[1].cluster) == 4163 and (want[1].total == 1).all()


def test_consensus_ties_at_depth_go_to_the_allele_shown_first():
    for alleles, n_alleles in (((0, 1), 2), ((14, 15), 16)):
        cases = pc.tie_cases(alleles, n_alleles)
        pc.check_ties(pt.threading_inputs_batch([pc.problem_of(c) for c in cases], host=True), cases, alleles)


def test_selection_at_the_exact_threshold():
    pc.check_exact_thresholds(lambda depths, ploidy: pt.select_clusters(depths, ploidy, 0, host=True))


@pytest.mark.parametrize("ploidy", [2, 6, 16])
def test_haplotypes_on_seeded_paths_equal_the_restatement(ploidy):
    blocks = pc.haplotype_blocks(ploidy)
    got, _ = host_and_restatement(blocks)
    pc.check_haplotypes(got, blocks, lambda paths, res: pt.haplotypes_from_inputs(paths, res, host=True))


def test_without_a_device_the_native_call_raises():
    """No CPU fallback: the product library's call either runs on a device or raises."""
    if _native.device_count() > 0:
        assert pt.threading_inputs_batch([tiny()])[0].tobytes() == pt.threading_inputs_batch([tiny()], host=True)[0].tobytes()
        return
    with pytest.raises(_native.SolverError) as e:
        pt.threading_inputs_batch([tiny()])
    assert e.value.status == _native.WHAMD_ERR_DEVICE
