"""CPU: haplotagphase (whatshap_amd.haplotagphase) on one host thread of the debug library against what the reference's compute_votes and
consensus recorded for every case of tests/haplotagphase_cases.py -- identical in every field: the votes dict with its order, both
superreads, the components with their order, the number of skipped reads; the reference's exception class where it raises."""
import random
import subprocess

import numpy as np
import pytest

import haplotagphase_cases as hc
from whatshap_amd import _native
from whatshap_amd import haplotagphase as tp

GOLDEN = {c["spec"]["name"]: c for c in hc.load_golden()["cases"]}
SPECS = {s["name"]: s for s in hc.all_specs()}
ERRORS = {"KeyError": KeyError, "ZeroDivisionError": ZeroDivisionError}
COUNTS = ("n_reads", "n_variants", "n_entries", "n_voting", "n_skipped", "n_voted", "n_kept", "n_zero_total", "variants_class_a", "variants_class_b",
          "variants_class_c", "variants_many_phase_sets", "table_rows")


def consensus_args(spec, args):
    return (spec["only_indels"], spec["gap_threshold"], spec["cut_homopolymers"], args["refseq"], args["change"], args["phased"])


def test_every_spec_is_recorded_and_generates_the_recorded_input():
    assert sorted(GOLDEN) == sorted(SPECS)
    for name, spec in SPECS.items():
        assert hc.input_sha256(hc.materialize(spec)) == GOLDEN[name]["input_sha256"], name
        assert GOLDEN[name]["raises"] == spec["expect_error"], name
    assert sum(1 for c in GOLDEN.values() if c["raises"]) == 4
    assert sum(1 for s in SPECS.values() if s["kind"] == "random") >= 24
    # the homopolymer cases: the recorded superreads do not depend on cut_homopolymers
    kept = {name: c["results"]["super_reads"] for name, c in GOLDEN.items() if name.startswith("homopolymer_cut_")}
    assert len(kept) == 6 and all(v == kept["homopolymer_cut_0"] and len(v[0]) == 6 for v in kept.values())


@pytest.mark.parametrize("name", [n for n, s in SPECS.items() if not s["expect_error"]])
def test_host_twin_equals_the_reference(name):
    spec = SPECS[name]
    want = GOLDEN[name]["results"]
    args = hc.call_args(hc.materialize(spec))
    skipped, stats = [], []
    votes = tp.compute_votes(args["is_homozygous"], args["reads"], args["allele_to_id"], host=True, skipped=skipped, stats=stats)
    super_reads, components = tp.consensus(*consensus_args(spec, args), votes, args["id_to_allele"])
    assert hc.canonical(votes, super_reads, components, skipped[0]) == want
    assert all(type(s) is int for vote in votes.values() for s in vote.values())
    (fused_reads, fused_components), fused_skipped = tp.votes_and_consensus(args["is_homozygous"], args["reads"], args["allele_to_id"], *consensus_args(spec, args),
                                                                            args["id_to_allele"], host=True, stats=stats)
    assert hc.canonical(votes, fused_reads, fused_components, fused_skipped) == want
    assert all(s["launches"] == 0 for s in stats) and stats[0]["table_rows"] == sum(len(v) // 2 for v in votes.values()) and stats[1]["table_rows"] == 0


@pytest.mark.parametrize("name", [n for n, s in SPECS.items() if not s["expect_error"]])
def test_array_level_call_equals_the_reference(name):
    """tagphase_batch on the arrays: every per-variant field against what the recorded votes dict implies."""
    spec = SPECS[name]
    want = GOLDEN[name]["results"]
    args = hc.call_args(hc.materialize(spec))
    p = tp.TagphaseProblem.from_reads(args["is_homozygous"], args["reads"], args["allele_to_id"], args["phased"], args["change"], spec["gap_threshold"],
                                      spec["only_indels"])
    with_table, without = tp.tagphase_batch([p, p], host=True, want_table=True)[0], tp.tagphase_batch([p], host=True)[0]
    for field in tp.TagphaseResult.FIELDS:
        assert np.array_equal(getattr(with_table, field), getattr(without, field)), field
    res = with_table
    order = res.order().tolist()
    assert [p.positions[x] for x in order] == [pos for pos, _ in want["votes"]]
    kept = {pos for pos, _, _ in want["super_reads"][0]}
    for x, (pos, vote) in zip(order, want["votes"]):
        rows = range(int(res.row_ptr[x]), int(res.row_ptr[x + 1]))
        got = [[int(res.row_ps[r]), h, int((res.row_sum0, res.row_sum1)[h][r])] for r in rows for h in (0, 1)]
        assert got == vote, pos
        assert res.n_phasesets[x] == len(vote) // 2 and res.total[x] == sum(s for _, _, s in vote)
        assert (int(res.best_ps[x]), int(res.best_id[x]), int(res.score[x])) == tuple(max(vote, key=lambda e: e[2])), pos   # (max: the first among equals)
        assert bool(res.kept[x]) == (pos in kept) and not res.zero_total[x]
        assert [int(res.first[x])] == [int(f) for f in res.row_first[rows.start:rows.start + 1]]
        assert np.all(np.diff(res.row_first[rows.start:rows.stop].astype(np.int64)) > 0)
    assert [[p.positions[x], int(res.best_ps[x])] for x in order] == want["components"]
    assert res.n_skipped == want["skipped"] and int(res.voted.sum()) == len(order)
    assert not res.voted[(p.variant_flags & tp.HOMOZYGOUS) != 0].any()


@pytest.mark.parametrize("name", [n for n, s in SPECS.items() if s["expect_error"]])
def test_exceptions_match_the_reference(name):
    spec, rec = SPECS[name], GOLDEN[name]
    args = hc.call_args(hc.materialize(spec))
    error = ERRORS[rec["raises"]]
    with pytest.raises(error):
        tp.votes_and_consensus(args["is_homozygous"], args["reads"], args["allele_to_id"], *consensus_args(spec, args), args["id_to_allele"], host=True)
    if rec["raised_by"] == "compute_votes":
        with pytest.raises(error):
            tp.compute_votes(args["is_homozygous"], args["reads"], args["allele_to_id"], host=True)
        return
    skipped = []
    votes = tp.compute_votes(args["is_homozygous"], args["reads"], args["allele_to_id"], host=True, skipped=skipped)   # (never raises for a zero total)
    assert hc.canonical(votes, [[], []], {}, skipped[0]) == rec["results"]
    with pytest.raises(error):
        tp.consensus(*consensus_args(spec, args), votes, args["id_to_allele"])
    p = tp.TagphaseProblem.from_reads(args["is_homozygous"], args["reads"], args["allele_to_id"])
    res = tp.tagphase_batch([p], host=True)[0]
    assert res.zero_total.sum() == 1 and not res.kept[res.zero_total != 0].any() and res.stats["n_zero_total"] == 1


def test_missing_phased_and_change_raise_key_error_where_the_reference_asks_them():
    spec = SPECS["only_indels_1"]
    args = hc.call_args(hc.materialize(spec))
    call = lambda **kw: tp.votes_and_consensus(args["is_homozygous"], args["reads"], args["allele_to_id"], *consensus_args(spec, dict(args, **kw)),  # noqa: E731
                                               args["id_to_allele"], host=True)
    with pytest.raises(KeyError):
        call(phased={k: v for k, v in args["phased"].items() if k != 20})
    with pytest.raises(KeyError):
        call(change={k: v for k, v in args["change"].items() if k != 20})
    call(change={k: v for k, v in args["change"].items() if k != 40})   # position 40 is phased: change[40] is never asked


def ok_arrays():
    return dict(variant_flags=[0, tp.SNV, tp.HOMOZYGOUS], read_ptr=[0, 2, 4], entry_variant=[0, 1, 1, 2], entry_id=[0, 1, 1, 0], entry_quality=[5, 6, 7, 8],
                read_ps=[10, 10], read_hp=[0, 1])


def test_unsupported_beyond_2_to_53():
    """The magnitudes of the voting entries may sum to 2^53 and no further.  A CSR cannot list an entry twice, so the few entries of quality
    2^31 - 1 are tiled: 2^22 of them stay below 2^53, a handful more of them cross it; entries that do not vote do not count."""
    big = (1 << 31) - 1
    for extra, hp, flags, refused in ((0, 0, 0, False), (8, 0, 0, True), (8, 2, 0, False), (8, 0, tp.HOMOZYGOUS, False)):
        n = (1 << 22) + extra
        assert (n * big > 1 << 53) == (extra > 0)
        reads = 4
        ptr = [0] + [n // reads * k for k in range(1, reads)] + [n]
        p = tp.TagphaseProblem([flags, 0], ptr, np.zeros(n, dtype=np.uint32), np.tile(np.array([0, 1, 0, 1], dtype=np.uint8), n // 4),
                               np.tile(np.array([big, -big, big, -big], dtype=np.int32), n // 4), [7] * reads, [hp] * reads)
        for host in (True, False):   # (the product library refuses before it looks for a device)
            if refused:
                with pytest.raises(_native.SolverError, match="2\\^53") as e:
                    tp.tagphase_batch([p], host=host)
                assert e.value.status == _native.WHAMD_ERR_UNSUPPORTED
            elif host or hp == 2 or flags:
                res = tp.tagphase_batch([p], host=host)[0]
                assert res.stats["n_voting"] == (0 if hp == 2 or flags else n)
                if res.stats["n_voting"]:
                    assert (int(res.score[0]), int(res.total[0]), bool(res.zero_total[0])) == (n // 2 * big, 0, True)


def test_native_validation_of_arrays():
    """Errors the native library finds in the arrays (nothing is launched: the device is never opened), from both libraries."""
    ok = ok_arrays()
    res = tp.tagphase_batch([tp.TagphaseProblem(**ok)], host=True, want_table=True)[0]
    assert res.voted.tolist() == [1, 1, 0] and res.score.tolist() == [5, 7, 0] and res.best_id.tolist() == [0, 0, 0] and res.first.tolist()[:2] == [0, 1]
    assert res.first[2] == tp.NOT_VOTED and res.row_ptr.tolist() == [0, 1, 2, 2] and res.row_sum1.tolist() == [0, 6] and res.row_sum0.tolist() == [5, 7]
    for change, match in ((dict(entry_variant=[0, 1, 3, 2]), "out of range"), (dict(entry_id=[0, 2, 1, 0]), "outside \\{0, 1\\}"), (dict(variant_flags=[0, 8, 1]), "bit 2"),
                          (dict(read_ptr=[0, 3, 2, 4], read_ps=[1, 1, 1], read_hp=[0, 0, 0]), "decreases"), (dict(read_ptr=[1, 2, 4]), "start at 0"),
                          (dict(gap_threshold=float("nan")), "NaN")):
        for host in (True, False):
            with pytest.raises(ValueError, match=match):
                tp.tagphase_batch([tp.TagphaseProblem(**dict(ok, **change))], host=host)
    with pytest.raises(ValueError, match="problem 1"):
        tp.tagphase_batch([tp.TagphaseProblem(**ok), tp.TagphaseProblem(**dict(ok, entry_id=[0, 1, 1, 9]))], host=True)
    for change, match in ((dict(entry_quality=[5, 6, 7, 1 << 31]), "int32"), (dict(entry_variant=[0, 1, -1, 2]), "out of range"), (dict(read_hp=[0]), "mismatched"),
                          (dict(entry_id=[0, 1, 1]), "mismatched")):
        with pytest.raises(ValueError, match=match):
            tp.TagphaseProblem(**dict(ok, **change))


def test_calls_without_a_voting_entry_never_reach_a_device():
    """The product library: nothing votes, nothing touches the device -- the call succeeds on a machine without one."""
    quiet = tp.TagphaseProblem(**dict(ok_arrays(), read_hp=[-1, 2]))
    for problems in ([], [quiet], [tp.TagphaseProblem([], [0], [], [], [], [], [])]):
        for res in tp.tagphase_batch(problems, want_table=True):
            assert res.stats["launches"] == 0 and not res.voted.any() and res.row_ps.size == 0
    assert tp.tagphase_batch([quiet])[0].n_skipped == 1


@pytest.mark.skipif(_native.device_count() > 0, reason="only meaningful on a machine without a GPU")
def test_without_a_device_the_native_call_raises():
    with pytest.raises(_native.SolverError) as e:
        tp.tagphase_batch([tp.TagphaseProblem(**ok_arrays())])
    assert e.value.status == _native.WHAMD_ERR_DEVICE


def test_the_new_exports_follow_the_export_rule():
    names = [n for n in _native.EXPORTED_SYMBOLS if n.startswith("whamd_tagphase")]
    assert len(names) == 8
    for path, debug in ((_native.LIB_PATH, False), (_native.DEBUG_LIB_PATH, True)):
        exported = {ln.split()[-1] for ln in subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout.splitlines() if ln.strip()}
        assert set(names) <= exported and all(n.startswith("whamd_") for n in exported)
        assert ("whamd_debug_tagphase_host" in exported) == debug


def test_plain_python_mirrors():
    assert tp.best_candidate({(1, 2): 50, (2, 3): 100, (3, 4): 75}) == (3, 2, 0.4444444444444444, 100)
    assert tp.best_candidate({(1, 2): 100, (2, 2): 100, (3, 3): 100}) == (2, 1, 0.3333333333333333, 100)
    assert tp.best_candidate({(0, 0): 2}) == (0, 0, 1.0, 2)
    with pytest.raises(ZeroDivisionError):
        tp.best_candidate({(0, 0): 0, (0, 1): 0})
    assert [tp.length_of_homopolymer(*a) for a in (("AAABBBCCC", 0, 1, 10), ("AAABBBCCC", 2, -1, 10), ("AAABBBCCC", 3, 1, 2), ("A", 0, 1, 1), ("AABBBCCCC", 5, 1, 5),
                                                   ("", 0, 1, 10))] == [3, 3, 2, 1, 4, 0]
    rng = random.Random(5)   # the filter asks for a length above the threshold the function stops at
    for _ in range(2000):
        ref = "".join(rng.choice("AAC") for _ in range(rng.randrange(0, 30)))
        threshold = rng.randrange(0, 12)
        assert tp.length_of_homopolymer(ref, rng.randrange(0, max(1, len(ref))), rng.choice((1, -1)), threshold) <= threshold


def test_stats_of_the_host_twin_follow_the_run_lengths():
    runs = [0, 1, 2, 64, 65, 4096, 4097, 7, 0, 300]
    p = hc.array_problem(runs, seed=3, n_phasesets=6)
    stats = []
    res = tp.tagphase_batch([p], host=True, stats=stats)[0]
    s = stats[0]
    assert s["n_voting"] == sum(runs) and s["n_voted"] == int(res.voted.sum()) == 8 and s["n_variants"] == len(runs) + 3
    assert (s["variants_class_a"], s["variants_class_b"], s["variants_class_c"]) == (4, 3, 1)
    assert s["variants_many_phase_sets"] == int((res.n_phasesets > 4).sum()) >= 5 and s["launches"] == 0 and s["n_skipped"] > 0
