"""GPU: haplotagphase (whatshap_amd.haplotagphase, csrc/tagphase_device.hip) against every recorded reference case and, on problems the
reference was not run on, against the one-thread host twin of the debug library: identical in every field, the counts of the stats
included; the launch constant; two calls on one input byte for byte."""
import os
import re

import numpy as np
import pytest

import haplotagphase_cases as hc
from whatshap_amd import haplotagphase as tp

pytestmark = pytest.mark.gpu

GOLDEN = {c["spec"]["name"]: c for c in hc.load_golden()["cases"]}
SPECS = {s["name"]: s for s in hc.all_specs()}
COUNTS = ("n_reads", "n_variants", "n_entries", "n_voting", "n_skipped", "n_voted", "n_kept", "n_zero_total", "variants_class_a", "variants_class_b",
          "variants_class_c", "variants_many_phase_sets", "table_rows")
_HEADER = open(os.path.join(os.path.dirname(os.path.abspath(tp.__file__)), "csrc", "tagphase.h")).read()


def constant(name):
    return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, _HEADER).group(1))


A_MAX, B_MAX, SEGMENT, R = constant("TP_CLASS_A_MAX"), constant("TP_CLASS_B_MAX"), constant("TP_SEGMENT"), constant("TP_REG_PHASESETS")
LAUNCHES, LAUNCHES_TABLE = constant("TP_LAUNCHES"), constant("TP_LAUNCHES_TABLE")


def same(got, want, table):
    for field in tp.TagphaseResult.FIELDS + (tp.TagphaseResult.TABLE_FIELDS if table else ()):
        assert np.array_equal(getattr(got, field), getattr(want, field)), field
    assert {k: got.stats[k] for k in COUNTS} == {k: want.stats[k] for k in COUNTS}


def device_and_host(problems, want_table=True):
    dev = tp.tagphase_batch(problems, want_table=want_table)
    host = tp.tagphase_batch(problems, host=True, want_table=want_table)
    for d, h in zip(dev, host):
        same(d, h, want_table)
        assert d.stats["launches"] in (0, LAUNCHES_TABLE if want_table else LAUNCHES)
    return dev


def consensus_args(spec, args):
    return (spec["only_indels"], spec["gap_threshold"], spec["cut_homopolymers"], args["refseq"], args["change"], args["phased"])


def test_device_equals_the_reference_on_every_recorded_case():
    problems = []
    for name, spec in SPECS.items():
        args = hc.call_args(hc.materialize(spec))
        if GOLDEN[name]["raises"] == "KeyError":
            continue
        want = GOLDEN[name]["results"]
        skipped = []
        votes = tp.compute_votes(args["is_homozygous"], args["reads"], args["allele_to_id"], skipped=skipped)
        if spec["expect_error"]:
            assert hc.canonical(votes, [[], []], {}, skipped[0]) == want, name
            with pytest.raises(ZeroDivisionError):
                tp.votes_and_consensus(args["is_homozygous"], args["reads"], args["allele_to_id"], *consensus_args(spec, args), args["id_to_allele"])
        else:
            (super_reads, components), n_skipped = tp.votes_and_consensus(args["is_homozygous"], args["reads"], args["allele_to_id"], *consensus_args(spec, args),
                                                                          args["id_to_allele"])
            assert hc.canonical(votes, super_reads, components, n_skipped) == want, name
            assert skipped[0] == n_skipped
        problems.append(tp.TagphaseProblem.from_reads(args["is_homozygous"], args["reads"], args["allele_to_id"], args["phased"], args["change"],
                                                      spec["gap_threshold"], spec["only_indels"]))
    device_and_host(problems)   # every field and the stats, all cases as one batch
    device_and_host(problems, want_table=False)


BOUNDARY_RUNS = [0, 1, 2, SEGMENT - 1, SEGMENT, SEGMENT + 1, A_MAX - 1, A_MAX, A_MAX + 1, 127, 128, 129, B_MAX - 1, B_MAX, B_MAX + 1, 50_021, 3, 0, 17]


@pytest.mark.parametrize("n_phasesets", [R - 1, R, R + 1])
def test_run_lengths_and_phase_set_counts_at_every_boundary(n_phasesets):
    """Variant v gets exactly BOUNDARY_RUNS[v] voting entries from reads of n_phasesets phase sets: a run of a few dozen entries meets all."""
    p = hc.array_problem(BOUNDARY_RUNS, seed=11 + n_phasesets, n_phasesets=n_phasesets)
    res = device_and_host([p])[0]
    s = res.stats
    assert s["n_voting"] == sum(BOUNDARY_RUNS) and s["launches"] == LAUNCHES_TABLE
    assert (s["variants_class_a"], s["variants_class_b"], s["variants_class_c"]) == (9, 6, 2)
    assert int(res.n_phasesets[:len(BOUNDARY_RUNS)].max()) == n_phasesets
    many = s["variants_many_phase_sets"]
    assert many >= 9 if n_phasesets > R else many == 0
    without = device_and_host([p], want_table=False)[0]
    for field in tp.TagphaseResult.FIELDS:
        assert np.array_equal(getattr(without, field), getattr(res, field)), field
    assert without.stats["launches"] == LAUNCHES


def test_waves_of_a_workgroup_that_meet_different_phase_sets():
    """One workgroup per deep variant: the entries arrive in the order of the reads, whose phase sets change along the way (sixteen
    stretches, about eight per deep variant, so every wave's part of the run has at most R of its own and all parts together more); and parts that share theirs."""
    apart = hc.array_problem([19_990, 5, 19_000], seed=5, n_phasesets=16, ps_in_order=True, n_homozygous=0, p_idle_reads=0.0)
    shared = hc.array_problem([30_000, B_MAX + 1], seed=6, n_phasesets=R, ps_in_order=True)
    dev = device_and_host([apart, shared])
    assert dev[0].stats["variants_class_c"] == 2 and dev[0].stats["variants_many_phase_sets"] == 2 and dev[0].n_phasesets.tolist() == [9, 1, 8]
    assert dev[1].stats["variants_class_c"] == 2 and dev[1].stats["variants_many_phase_sets"] == 0


EDGE_READ_LENGTHS = (0, 255, 0, 0, 1, 1, 0, 343, 0)


def edge_reads_problem(n_entries):
    """The reads around a workgroup's edge (256 entries per workgroup in the count and place launches), from arrays: entries 255 and 256
    are single-entry reads with empty reads before, between and behind; cut at n_entries (the reads behind the cut stay, empty).  Every
    read votes: twenty heterozygous variants, R + 1 phase sets."""
    rng = np.random.default_rng(600 + n_entries)
    read_ptr = np.minimum(np.concatenate([[0], np.cumsum(EDGE_READ_LENGTHS)]), n_entries).astype(np.uint64)
    n_reads = len(EDGE_READ_LENGTHS)
    flags = rng.choice(np.array([0, tp.PHASED, tp.SNV, tp.PHASED | tp.SNV], dtype=np.uint8), size=20)
    tags = rng.integers(0, 1 << 40, size=R + 1, dtype=np.int64)
    read_ps = tags[[R, 0, R, 2, 1, 2, 3, 3, 0]]   # (the four reads with entries carry four of them)
    return tp.TagphaseProblem(flags, read_ptr, rng.integers(0, 20, size=n_entries), rng.integers(0, 2, size=n_entries),
                              rng.integers(1, 61, size=n_entries, dtype=np.int64), read_ps, rng.integers(0, 2, size=n_reads).astype(np.int32), 60.0, False)


@pytest.mark.parametrize("n_entries", [1, 256, 257, 600])
@pytest.mark.parametrize("want_table", [False, True])
def test_reads_at_a_workgroup_edge(n_entries, want_table):
    """The read lookup where a workgroup's 256 entries end, and the same reads cut to 1, 256 and 257 entries."""
    res = device_and_host([edge_reads_problem(n_entries)], want_table=want_table)[0]
    s = res.stats
    assert s["n_reads"] == len(EDGE_READ_LENGTHS) and s["n_entries"] == s["n_voting"] == n_entries
    assert s["launches"] == (LAUNCHES_TABLE if want_table else LAUNCHES)
    assert int(res.n_phasesets.max()) >= (2 if n_entries == 600 else 1)   # (the two long reads carry different phase sets)


def three_reads_problem(seed, votes=True):
    """Three reads of two entries each over four variants; without `votes` every variant is homozygous, so no entry votes."""
    rng = np.random.default_rng(seed)
    flags = rng.choice(np.array([0, tp.PHASED, tp.SNV, tp.PHASED | tp.SNV], dtype=np.uint8), size=4) | (0 if votes else tp.HOMOZYGOUS)
    tags = rng.integers(0, 1 << 40, size=2, dtype=np.int64)
    return tp.TagphaseProblem(flags.astype(np.uint8), np.array([0, 2, 4, 6], dtype=np.uint64), rng.integers(0, 4, size=6), rng.integers(0, 2, size=6),
                              rng.integers(1, 61, size=6, dtype=np.int64), tags[[0, 1, 0]], np.array([0, 1, 1], dtype=np.int32), 60.0, False)


def test_problems_with_a_table_without_one_and_without_a_vote_in_one_call():
    """One call whose problems want a table, want none, have no voting entry, and want a table again: the rows of the two tables lie one
    after the other in the call's rows, behind the rows of the problem that wants none.  Byte for byte the host twin's."""
    problems = [three_reads_problem(1), three_reads_problem(2), three_reads_problem(3, votes=False), three_reads_problem(4)]
    wants = [True, False, False, True]
    dev = tp.tagphase_batch(problems, want_table=wants)
    host = tp.tagphase_batch(problems, host=True, want_table=wants)
    for d, h, want in zip(dev, host, wants):
        for field in tp.TagphaseResult.FIELDS + (tp.TagphaseResult.TABLE_FIELDS if want else ()):
            assert getattr(d, field).tobytes() == getattr(h, field).tobytes(), field
        assert {k: d.stats[k] for k in COUNTS} == {k: h.stats[k] for k in COUNTS}
        assert d.stats["launches"] == LAUNCHES_TABLE
    assert dev[0].stats["table_rows"] > 0 and dev[3].stats["table_rows"] > 0 and dev[2].stats["n_voting"] == 0 and dev[1].stats["n_voting"] > 0


def test_two_calls_on_one_input_give_identical_bytes():
    """The order inside a run is whatever the atomics gave; it must not show."""
    p = hc.array_problem(hc.heavy_tail_runs(3_000, seed=8, mean=20, tail=0.01, tail_max=9_000), seed=9, n_phasesets=5, quality=(1, 2))
    first, second = (tp.tagphase_batch([p], want_table=True)[0] for _ in range(2))
    for field in tp.TagphaseResult.FIELDS + tp.TagphaseResult.TABLE_FIELDS:
        assert getattr(first, field).tobytes() == getattr(second, field).tobytes(), field
    same(first, tp.tagphase_batch([p], host=True, want_table=True)[0], True)


def test_many_small_problems_in_one_call_take_the_constant_number_of_launches():
    rng = np.random.default_rng(41)
    problems = []
    for k in range(1000):
        if k % 97 == 17:
            runs = []                          # a problem without variants that vote
        elif k % 97 == 40:
            runs = [0, 0, 0]
        else:
            runs = rng.integers(0, 6, size=int(rng.integers(1, 8)))
        problems.append(hc.array_problem(runs, seed=100 + k, n_phasesets=1 + k % 6, mean_read=3, n_homozygous=k % 3, gap_threshold=float(40 + k % 50),
                                         only_indels=bool(k & 1)))
    batch = device_and_host(problems)
    assert all(b.stats["launches"] == LAUNCHES_TABLE for b in batch)
    for k in (0, 17, 40, 500, 999):
        alone = tp.tagphase_batch([problems[k]], want_table=True)[0]
        same(alone, batch[k], True)
        assert alone.stats["launches"] == (0 if k in (17, 40) else LAUNCHES_TABLE)
    assert all(b.stats["launches"] == LAUNCHES for b in tp.tagphase_batch(problems))


def test_a_million_entries_with_heavy_tailed_coverage():
    runs = hc.heavy_tail_runs(30_000, seed=21, mean=30, tail=0.001, tail_max=20_000)
    p = hc.array_problem(runs, seed=22, n_phasesets=6, mean_read=25)
    without = device_and_host([p], want_table=False)[0]
    s = without.stats
    assert s["n_entries"] > 1_000_000 and s["n_voting"] == int(runs.sum()) and s["launches"] == LAUNCHES
    assert s["variants_class_a"] > 20_000 and s["variants_class_b"] > 1_000 and s["variants_class_c"] > 10 and s["variants_many_phase_sets"] > 10_000
    with_table = tp.tagphase_batch([p], want_table=True)[0]
    for field in tp.TagphaseResult.FIELDS:
        assert np.array_equal(getattr(with_table, field), getattr(without, field)), field
    assert with_table.stats["table_rows"] == int(without.n_phasesets.sum()) == with_table.row_ps.size


def test_more_scan_tiles_than_one_pass_of_the_second_scan_launch():
    """2048 * 512 + 1 variants are 513 scan tiles: the one workgroup that scans the tile totals takes 256 per pass, so it carries over
    twice and its last pass holds a single tile with a single variant.  Almost every variant is empty.  Voting entries lie on both sides
    of the first tile's end (2047 | 2048), of the first pass's end (524 287 | 524 288) and of the last full tile's end (1 048 575 |
    1 048 576); a class b and a class c run lie inside the last full tile, so their list entries, and the run begins behind them, come
    from the second pass.  The idle reads' entries, which do not vote, fall anywhere."""
    n_var, last_full = 2048 * 512 + 1, 2048 * 511
    runs = np.zeros(n_var, dtype=np.int64)
    runs[[0, 2047, 2048, 2049, 524_287, 524_288, 1_048_575, 1_048_576]] = [3, 1, 2, 5, 7, 1, 4, 6]
    runs[last_full + 100], runs[last_full + 1000] = A_MAX + 1, B_MAX + 1
    p = hc.array_problem(runs, seed=77, n_phasesets=R + 1, n_homozygous=0)
    for want_table in (True, False):
        s = device_and_host([p], want_table=want_table)[0].stats
        assert s["n_variants"] == n_var and s["n_voting"] == int(runs.sum()) and s["n_voted"] == 10
        assert (s["variants_class_b"], s["variants_class_c"]) == (1, 1)
        assert s["launches"] == (LAUNCHES_TABLE if want_table else LAUNCHES)


def test_calls_without_a_voting_entry_launch_nothing():
    empty = hc.array_problem([], seed=1, n_homozygous=0)   # (no variants at all)
    hollow = hc.array_problem([0, 0, 0, 0], seed=2)
    for problems in ([], [empty], [hollow], [empty, hollow, empty]):
        for res in tp.tagphase_batch(problems, want_table=True):
            assert res.stats["launches"] == 0 and res.stats["n_voted"] == 0 and not res.voted.any()
