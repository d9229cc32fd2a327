"""CPU: allele detection by re-alignment, host side.  The debug library's restatement (the CIGAR walk and windows of csrc/realign.cpp,
then both distances and the decision on one host thread) against every recorded yield of the reference
(tests/golden/make_realign_golden.py), and every exception the reference raises."""
import pytest

from realign_cases import group_objects, load
from whatshap_amd import realign

CASES = load()
EXCEPTIONS = {"ValueError": ValueError, "AssertionError": AssertionError, "IndexError": IndexError, "TypeError": TypeError}


def run_group(g, host=True):
    variants, restricted, reads, js = group_objects(g)
    kw = dict(g["params"])
    got = []
    for read, j, want in zip(reads, js, g["expected"]):
        if isinstance(want, dict):
            with pytest.raises(EXCEPTIONS[want["error"]]):
                realign.detect_alleles_batch(variants, [read], g["reference"], restricted, first_variant=[j], host=host, **kw)
            got.append(want)
        else:
            got.append([list(t) for t in realign.detect_alleles_batch(variants, [read], g["reference"], restricted, first_variant=[j], host=host, **kw)[0]])
    return got


@pytest.mark.parametrize("k", range(len(CASES["groups"])))
def test_host_walk_and_decision_equal_reference(k):
    g = CASES["groups"][k]
    assert run_group(g) == g["expected"]


def test_host_batch_equals_per_read():
    """The batch of all error-free reads of a group in one call gives the per-read lists."""
    checked = 0
    for g in CASES["groups"]:
        variants, restricted, reads, js = group_objects(g)
        keep = [i for i, e in enumerate(g["expected"]) if isinstance(e, list)]
        got = realign.detect_alleles_batch(variants, [reads[i] for i in keep], g["reference"], restricted, first_variant=[js[i] for i in keep],
                                           host=True, **g["params"])
        assert [[list(t) for t in x] for x in got] == [g["expected"][i] for i in keep]
        checked += len(keep)
    assert checked > 400


def test_host_distances_equal_reference():
    pairs = CASES["pairs"]
    unit = [p for p in pairs if "unit" in p]
    got = realign.edit_distance_batch([(p["q"], p["t"]) for p in unit], host=True)
    assert got.tolist() == [p["unit"] for p in unit]
    for gap in ((1, 1), (10, 7), (10.5, 7)):
        aff = [p for p in pairs if "affine" in p and tuple(p["gap"]) == gap]
        assert aff
        got = realign.edit_distance_affine_gap_batch([(p["q"], p["t"], p["costs"]) for p in aff], gap[0], gap[1], host=True)
        assert got.tolist() == [p["affine"] for p in aff]


def test_error_messages():
    from realign_cases import Aln, Var

    ref = "ACGTACGTAC" * 8
    v = [Var(30, "G", ["T"])]
    with pytest.raises(ValueError, match="Unsupported CIGAR operation: 9"):
        realign.detect_alleles_batch(v, [Aln(20, [(0, 5), (9, 3)], ref[20:28])], ref, host=True)
    with pytest.raises(IndexError):
        realign.detect_alleles_batch(v, [Aln(20, [(0, 15)], ref[20:35])], ref, [[5]], host=True)
    with pytest.raises(AssertionError):
        realign.detect_alleles_batch([Var(35, "A", ["C"]), Var(22, "G", ["T"])], [Aln(20, [(0, 10), (0, 20)], ref[20:50])], ref, host=True)
    with pytest.raises(TypeError):
        realign.detect_alleles_batch(v, [Aln(20, [(0, 15)], None)], ref, host=True)
    # affine without its parameters: the reference's assert, only when a job is realigned
    with pytest.raises(AssertionError):
        realign.detect_alleles_batch(v, [Aln(20, [(0, 15)], ref[20:35])], ref, use_affine=True, host=True)
    assert realign.detect_alleles_batch(v, [Aln(20, [], ref[20:35])], ref, use_affine=True, host=True) == [[]]
    with pytest.raises(NotImplementedError):
        list(realign.detect_alleles_by_alignment(v, None, 0, Aln(20, [(0, 15)], ref[20:35]), ref, use_kmerald=True))
    with pytest.raises(NotImplementedError):
        realign.edit_distance("AC", "AG", maxdiff=3)


def test_affine_without_parameters_asserts_before_index_error():
    """realign asserts the gap parameters after slicing the query and before the distances: an empty allowed set behind it is not reached."""
    from realign_cases import Aln, Var

    ref = "ACGTACGTAC" * 8
    v = [Var(30, "G", ["T"])]
    with pytest.raises(AssertionError):
        realign.detect_alleles_batch(v, [Aln(20, [(0, 15)], ref[20:35])], ref, [[5]], use_affine=True, gap_start=10, host=True)
    with pytest.raises(TypeError):
        realign.detect_alleles_batch(v, [Aln(20, [(0, 15)], None)], ref, use_affine=True, host=True)


def test_first_variant_default_equals_bisect():
    """Without first_variant the walk starts at variant 0 (a binary search on a sorted list); with the bisect index of each read it gives the same."""
    import bisect

    checked = 0
    for g in CASES["groups"]:
        variants, restricted, reads, js = group_objects(g)
        keep = [i for i, e in enumerate(g["expected"]) if isinstance(e, list)]
        positions = [v.position for v in variants]
        if positions != sorted(positions):
            continue
        sel = [reads[i] for i in keep]
        a = realign.detect_alleles_batch(variants, sel, g["reference"], restricted, host=True, **g["params"])
        b = realign.detect_alleles_batch(variants, sel, g["reference"], restricted, first_variant=[bisect.bisect_left(positions, r.reference_start) for r in sel],
                                         host=True, **g["params"])
        assert a == b
        checked += len(sel)
    assert checked > 100
