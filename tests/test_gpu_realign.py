"""GPU: allele detection by re-alignment on the MI355X (csrc/realign_device.hip) against the reference's recorded yields and distances,
a plain Python restatement on random pairs (multi-word Myers, multi-strip Gotoh), and the debug library's host path on a batch of more
than a million jobs."""
import random

import numpy as np
import pytest

from realign_cases import (DETECT_DELETIONS, DETECT_INSERTIONS, DETECT_OVERHANG, EDGE_GAPS, affine_distance, detect_shape_case, group_objects, load, load_edge,
                           reuse_pairs, unit_distance)
from whatshap_amd import realign
from whatshap_amd.synthetic import realign_workload

pytestmark = pytest.mark.gpu
CASES = load()


def test_device_groups_equal_reference():
    for g in CASES["groups"]:
        variants, restricted, reads, js = group_objects(g)
        for read, j, want in zip(reads, js, g["expected"]):
            if isinstance(want, dict):
                with pytest.raises({"ValueError": ValueError, "AssertionError": AssertionError, "IndexError": IndexError, "TypeError": TypeError}[want["error"]]):
                    realign.detect_alleles_batch(variants, [read], g["reference"], restricted, first_variant=[j], **g["params"])
            else:
                got = list(realign.detect_alleles_by_alignment(variants, restricted, j, read, g["reference"], **g["params"]))
                assert [list(t) for t in got] == want
        keep = [i for i, e in enumerate(g["expected"]) if isinstance(e, list)]
        got = realign.detect_alleles_batch(variants, [reads[i] for i in keep], g["reference"], restricted, first_variant=[js[i] for i in keep], **g["params"])
        assert [[list(t) for t in x] for x in got] == [g["expected"][i] for i in keep]


def test_device_distances_equal_reference():
    pairs = CASES["pairs"]
    unit = [p for p in pairs if "unit" in p]
    assert realign.edit_distance_batch([(p["q"], p["t"]) for p in unit]).tolist() == [p["unit"] for p in unit]
    for gap in ((1, 1), (10, 7), (10.5, 7)):
        aff = [p for p in pairs if "affine" in p and tuple(p["gap"]) == gap]
        got = realign.edit_distance_affine_gap_batch([(p["q"], p["t"], p["costs"]) for p in aff], gap[0], gap[1])
        assert got.tolist() == [p["affine"] for p in aff]
    assert realign.edit_distance("ACGT", "AGT") == 1
    assert realign.edit_distance_affine_gap("ACGT", "AGT", [3.0] * 4, 10, 7) == 10


def random_pairs(n, seed):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        m = rng.randint(0, 300)
        s = "".join(rng.choice("ACGTN") for _ in range(m))
        t = list(s)
        for _ in range(rng.randint(0, 40)):
            p = rng.randint(0, len(t))
            r = rng.random()
            if r < 0.4 and p < len(t):
                t[p] = rng.choice("ACGTa")
            elif r < 0.7:
                t[p:p] = [rng.choice("ACGT") for _ in range(rng.randint(1, 10))]
            else:
                del t[p:p + rng.randint(1, 10)]
        t = "".join(t)[:300] if rng.random() < 0.9 else "".join(rng.choice("ACGT") for _ in range(rng.randint(0, 300)))
        costs = [rng.choice([15.1, 0.3, 2.5]) for _ in s]
        out.append((s, t, costs))
    return out


def test_device_random_pairs():
    pairs = random_pairs(20000, 7)
    unit = realign.edit_distance_batch([(s, t) for s, t, _ in pairs])
    assert unit.tolist() == realign.edit_distance_batch([(s, t) for s, t, _ in pairs], host=True).tolist()
    aff = realign.edit_distance_affine_gap_batch(pairs, 10, 7)
    assert aff.tolist() == realign.edit_distance_affine_gap_batch(pairs, 10, 7, host=True).tolist()
    assert max(len(s) for s, _, _ in pairs) > 256 and max(len(t) for _, t, _ in pairs) > 256
    for k in range(0, 20000, 1000):   # the Python restatement on a sample (it is slow)
        s, t, c = pairs[k]
        assert unit[k] == unit_distance(s.encode(), t.encode())
        assert aff[k] == affine_distance(s.encode(), t.encode(), c, 10, 7)


@pytest.mark.parametrize("use_affine", [False, True])
def test_device_large_batch_equals_host(use_affine):
    ref, variants, reads = realign_workload(n_variants=60_000, genome=5_000_000, coverage=20, seed=3)
    kw = dict(use_affine=use_affine, gap_start=10, gap_extend=7, default_mismatch=15.1) if use_affine else {}
    got, stats = realign.detect_alleles_batch(variants, reads, ref, with_stats=True, **kw)
    assert stats["n_jobs"] >= 1_000_000, stats
    want = realign.detect_alleles_batch(variants, reads, ref, host=True, **kw)
    assert got == want
    assert sum(len(x) for x in got) > 0.9 * stats["n_jobs"]


def test_empty_and_errors_without_launch():
    assert realign.detect_alleles_batch([], [], "ACGT") == []
    from realign_cases import Aln, Var

    ref = "ACGT" * 20
    assert realign.detect_alleles_batch([Var(5, "A", ["C"])], [Aln(40, [(0, 10)], ref[40:50])], ref) == [[]]
    with pytest.raises(ValueError, match="Unsupported CIGAR operation: 12"):
        realign.detect_alleles_batch([Var(30, "G", ["T"])], [Aln(20, [(0, 5), (12, 3)], ref[20:28])], ref)
    with pytest.raises(IndexError):
        realign.detect_alleles_batch([Var(30, "G", ["T"])], [Aln(20, [(0, 15)], ref[20:35])], ref, [[4]])
    assert realign.edit_distance_batch([]).tolist() == []


def test_device_long_targets_beyond_lds():
    """Queries longer than 64 against targets longer than 5 460 bytes: the affine strip boundary no longer fits in LDS and lives in a
    global scratch row; the unit carry rows are sized by these jobs alone."""
    rng = random.Random(11)
    pairs = []
    for n in (5461, 6000, 9000):
        t = "".join(rng.choice("ACGT") for _ in range(n))
        for m in (65, 130, 300):
            k = rng.randint(0, n - m)
            q = list(t[k:k + m])
            q[m // 2] = "N"
            pairs.append(("".join(q), t, [rng.choice([15.1, 0.3]) for _ in range(m)]))
    pairs += random_pairs(300, 12)   # short and long in one call
    assert realign.edit_distance_batch([(s, t) for s, t, _ in pairs]).tolist() == \
        realign.edit_distance_batch([(s, t) for s, t, _ in pairs], host=True).tolist()
    for gap in ((10, 7), (1, 1)):
        assert realign.edit_distance_affine_gap_batch(pairs, *gap).tolist() == realign.edit_distance_affine_gap_batch(pairs, *gap, host=True).tolist()


# ------------------------------------------------------------------------------------------------- every launch shape, every length edge
# The long jobs' launch (csrc/realign_shape.h, the table in DESIGN.md): each test below first holds, through the debug library's exports,
# the shape its call takes, then the device's result against the host twin (full matrix, no bit-parallel or anti-diagonal code) and the
# reference's recorded distances (tests/golden/realign_edge_cases.json.gz).  Everything is integer equality on every pair.
EDGE, EDGE_FIXTURE = load_edge()
AFFINE_KW = dict(use_affine=True, gap_start=10, gap_extend=7, default_mismatch=15.1)
SHAPE_OF_TARGET = {1364: "four-wave", 1365: "one-wave", 5460: "one-wave", 5461: "global"}


def affine_shape_name(s):
    assert s["lds_bytes"] <= 65536 and s["carry_words"] == 0
    if s["global_rows"]:
        assert s["block"] == 64 and s["lds_bytes"] == 0 and s["scratch_bytes"] == s["blocks"] * 4 * s["row_floats"]
        return "global"
    assert s["scratch_bytes"] == 0 and s["lds_bytes"] == (s["block"] // 64) * 4 * s["row_floats"]
    return {256: "four-wave", 64: "one-wave"}[s["block"]]


def pairs_shape(pairs, affine):
    """The shape of the long launch of an edit_distance*_batch over `pairs`, with the counts it was made from."""
    counts = realign.debug_pair_counts(pairs)
    s = realign.debug_long_shape(affine, counts["n_long"], counts["max_target_long"])
    assert s["blocks"] >= 1, "no long job in this call"
    if not affine:
        assert s["block"] == 64 and s["carry_words"] == 2 * ((counts["max_target_long"] + 63) // 64) and s["scratch_bytes"] == s["blocks"] * 512 * s["carry_words"]
    return dict(s, **counts)


def check_edge_pairs(idx, want_shape=None, want_target=None):
    """Unit and affine distances of the edge pairs `idx` in one call each (affine: one per gap pair) against the fixture and the host twin."""
    upairs = [(EDGE[k]["q"], EDGE[k]["t"]) for k in idx]
    s = pairs_shape(upairs, False)
    if want_target is not None:
        assert s["max_target_long"] == want_target
    got = realign.edit_distance_batch(upairs)
    assert got.tolist() == [EDGE_FIXTURE["unit"][k] for k in idx]
    assert got.tolist() == realign.edit_distance_batch(upairs, host=True).tolist()
    for gap in sorted({tuple(EDGE[k]["gap"]) for k in idx}):
        sel = [k for k in idx if tuple(EDGE[k]["gap"]) == gap]
        triples = [(EDGE[k]["q"], EDGE[k]["t"], EDGE[k]["costs"]) for k in sel]
        if not any(len(q) > 64 for q, _, _ in triples):
            continue
        s = pairs_shape(triples, True)
        if want_shape is not None:
            assert affine_shape_name(s) == want_shape, (gap, s)
        if want_target is not None and gap in EDGE_GAPS:   # (the pairs with gaps beyond 2^24 have targets of at most 300)
            assert s["max_target_long"] == want_target
        got = realign.edit_distance_affine_gap_batch(triples, *gap)
        assert got.tolist() == [EDGE_FIXTURE["affine"][k] for k in sel], gap
        assert got.tolist() == realign.edit_distance_affine_gap_batch(triples, *gap, host=True).tolist()


def test_edge_pairs_in_one_call():
    """Every edge pair in one call: the longest target of a long job is 5461, so every long job runs on global rows (and, unit, on carry rows
    of 172 words), the short job with the 5461-byte target in the launch without scratch."""
    idx = list(range(len(EDGE)))
    assert pairs_shape([(p["q"], p["t"]) for p in EDGE], False)["carry_words"] == 172
    for gap in ((10, 7), (1, 1)):
        assert affine_shape_name(pairs_shape([(p["q"], p["t"]) for p in EDGE if tuple(p["gap"]) == gap], True)) == "global"
    check_edge_pairs(idx)


@pytest.mark.parametrize("shape_name,lo,hi", [("four-wave", 0, 1364), ("one-wave", 1365, 5460), ("global", 5461, 1 << 30)])
def test_edge_pairs_grouped_by_shape(shape_name, lo, hi):
    """The same pairs grouped by target length, so that each call's longest target stays within one affine shape."""
    idx = [k for k, p in enumerate(EDGE) if lo <= len(p["t"]) <= hi and (len(p["q"]) > 64 or hi < 1 << 30)]
    assert idx and max(len(EDGE[k]["t"]) for k in idx) == min(hi, 5461)
    check_edge_pairs(idx, want_shape=shape_name, want_target=min(hi, 5461))
    if shape_name == "global":   # the short job with a long target, on its own: no second launch at all
        k = [k for k, p in enumerate(EDGE) if p["name"] == "shape-short-m64-n5461"]
        p = EDGE[k[0]]
        assert realign.debug_pair_counts([(p["q"], p["t"])]) == {"n_long": 0, "max_target_long": 0}
        assert realign.edit_distance_batch([(p["q"], p["t"])]).tolist() == [EDGE_FIXTURE["unit"][k[0]]]
        assert realign.edit_distance_affine_gap_batch([(p["q"], p["t"], p["costs"])], *p["gap"]).tolist() == [EDGE_FIXTURE["affine"][k[0]]]


@pytest.mark.parametrize("m", [65, 129, 300])
@pytest.mark.parametrize("max_target", [1364, 1365, 5460, 5461])
def test_one_call_per_shape_edge(max_target, m):
    """A call whose longest target is exactly max_target, for queries of m bytes, next to shorter pairs: 1364 is the last four-wave launch,
    1365 the first one-wave launch with its row in LDS, 5460 the last (a row of 65 532 bytes), 5461 the first with global rows."""
    idx = [k for k, p in enumerate(EDGE) if p["group"] == "shape" and len(p["t"]) == max_target and len(p["q"]) == m]
    assert len(idx) == 2
    idx += [k for k, p in enumerate(EDGE) if p["group"] in ("grid", "strip") and (len(p["q"]) in (64, m) or len(p["t"]) == 300)]
    check_edge_pairs(idx, want_shape=SHAPE_OF_TARGET[max_target], want_target=max_target)
    s = pairs_shape([(EDGE[k]["q"], EDGE[k]["t"]) for k in idx if tuple(EDGE[k]["gap"]) == (10, 7)], True)
    assert (s["block"], s["lds_bytes"], s["global_rows"]) == {1364: (256, 65520, 0), 1365: (64, 16392, 0), 5460: (64, 65532, 0), 5461: (64, 0, 1)}[max_target]


@pytest.mark.parametrize("shape_name,n_pairs,first_target", [("four-wave", 8300, 1364), ("one-wave", 2100, 1365), ("global", 2100, 5461)])
def test_affine_boundary_rows_are_reused(shape_name, n_pairs, first_target):
    """More long jobs than the launch has waves: a wave's later job runs on the boundary row an earlier one filled -- a longer one for every
    second wave, a shorter one for the others."""
    waves = 4096 if shape_name == "four-wave" else 1024
    pairs = reuse_pairs(n_pairs, waves, (65, 140), (120, 200), (40, 90), first_target, seed=len(shape_name))
    s = pairs_shape(pairs, True)
    assert affine_shape_name(s) == shape_name and s["max_target_long"] == first_target
    assert s["blocks"] == 1024 and s["blocks"] * s["block"] // 64 == waves and s["n_long"] == n_pairs >= 2 * waves
    for gap in ((10, 7), (1, 1)):
        assert realign.edit_distance_affine_gap_batch(pairs, *gap).tolist() == realign.edit_distance_affine_gap_batch(pairs, *gap, host=True).tolist()


def test_unit_carry_rows_are_reused():
    """More long jobs than the unit launch has lanes (65 536): a lane's second job runs on the carry row its first one filled, with one carry
    word more or less than it."""
    pairs = reuse_pairs(70000, 65536, (65, 70), (125, 135), (60, 72), 130, seed=4)
    s = pairs_shape(pairs, False)
    assert s["blocks"] == 1024 and s["n_long"] == 70000 > s["blocks"] * 64 and s["carry_words"] == 6
    pairs = [(q, t) for q, t, _ in pairs]
    assert realign.edit_distance_batch(pairs).tolist() == realign.edit_distance_batch(pairs, host=True).tolist()


@pytest.mark.parametrize("use_affine", [False, True])
@pytest.mark.parametrize("kind,size", [("del", n) for n in DETECT_DELETIONS] + [("ins", n) for n in DETECT_INSERTIONS])
def test_detect_at_the_shapes(kind, size, use_affine):
    """detect_alleles_batch with an indel whose longest window decides the shape: deletions whose reference window (allele 0) is exactly
    1364 / 1365 / 5460 / 5461 bytes, insertions whose alt window (allele 1: left | alt | right, three segments) is the longest.  Every job
    is a long job (overhang 40)."""
    c = detect_shape_case(kind, size)
    kw = dict(AFFINE_KW) if use_affine else {}
    counts = realign.debug_walk_counts(c["variants"], c["reads"], c["reference"], overhang=c["overhang"], **kw)
    assert counts == {"n_jobs": 8, "n_long": 8, "max_target_long": size if kind == "del" else 81 + size}
    s = realign.debug_long_shape(use_affine, counts["n_long"], counts["max_target_long"])
    if use_affine:
        assert affine_shape_name(s) == {1364: "four-wave", 1365: "one-wave", 5460: "one-wave", 5461: "global", 1481: "one-wave", 5581: "global"}[counts["max_target_long"]]
    else:
        assert s["blocks"] == 1 and s["carry_words"] == 2 * ((counts["max_target_long"] + 63) // 64)
    got = realign.detect_alleles_batch(c["variants"], c["reads"], c["reference"], overhang=c["overhang"], **kw)
    assert got == realign.detect_alleles_batch(c["variants"], c["reads"], c["reference"], overhang=c["overhang"], host=True, **kw)
    assert [[(v, a) for v, a, _ in x] for x in got] == c["alleles"]
    if not use_affine:
        assert {q for x in got for _, _, q in x} == {30}


@pytest.mark.parametrize("use_affine", [False, True])
def test_decision_of_long_jobs(use_affine):
    """realign's decision where the query is longer than 64: one allowed allele (taken whatever its distance), two alleles at equal distance
    (no decision), three alleles whose two worse distances tie (the best one; affine quality d0 - d1)."""
    from realign_cases import Aln, Var

    rng = random.Random(17)
    ref = "".join(rng.choice("ACG") for _ in range(600))   # (no T: a T in a read is neither the reference nor an alt below)
    ref = ref[:100] + "A" + ref[101:200] + "A" + ref[201:300] + "A" + ref[301:]
    variants = [Var(100, "A", ["C"]), Var(200, "A", ["C"]), Var(300, "A", ["C", "G"])]
    seq = ref[20:100] + "C" + ref[101:200] + "T" + ref[201:300] + "C" + ref[301:400]
    reads = [Aln(20, [(0, 380)], seq)]
    kw = dict(AFFINE_KW) if use_affine else {}
    restricted = [[0, 0], None, None]
    counts = realign.debug_walk_counts(variants, reads, ref, restricted, overhang=DETECT_OVERHANG, **kw)
    assert counts == {"n_jobs": 3, "n_long": 3, "max_target_long": 81}
    got = realign.detect_alleles_batch(variants, reads, ref, restricted, overhang=DETECT_OVERHANG, **kw)
    assert got == realign.detect_alleles_batch(variants, reads, ref, restricted, overhang=DETECT_OVERHANG, host=True, **kw)
    # variant 0: the read carries C, only allele 0 is allowed -> 0 (affine quality: its distance, one mismatch of 15.1); variant 1: T against A | C -> no
    # decision; variant 2: C -> allele 1 at distance 0, alleles 0 and 2 both one mismatch away (affine quality 0 - 15)
    assert got == [[(0, 0, 15), (2, 1, -15)]] if use_affine else got == [[(0, 0, 30), (2, 1, 30)]]


@pytest.mark.parametrize("use_affine", [False, True])
def test_device_long_deletion(use_affine):
    """A sequence-resolved deletion of 6 kb spanned by reads that carry the reference and by reads that carry the deletion."""
    from realign_cases import Aln, Var

    rng = random.Random(5)
    ref = "".join(rng.choice("ACGT") for _ in range(12000))
    pos, dl = 3000, 6000
    variants = [Var(2500, ref[2500], ["T" if ref[2500] != "T" else "A"]), Var(pos, ref[pos:pos + dl + 1], [ref[pos]]), Var(9500, ref[9500], ["G" if ref[9500] != "G" else "C"])]
    reads = [Aln(2000, [(0, 8000)], ref[2000:10000]),                                          # reference allele: a 6 kb window each way
             Aln(2000, [(0, 1001), (2, dl), (0, 999)], ref[2000:pos + 1] + ref[pos + dl + 1:10000]),   # the deletion
             Aln(2900, [(4, 20), (0, 6200)], "A" * 20 + ref[2900:9100])]
    kw = dict(use_affine=True, gap_start=10, gap_extend=7, default_mismatch=15.1) if use_affine else {}
    got = realign.detect_alleles_batch(variants, reads, ref, overhang=25, **kw)
    assert got == realign.detect_alleles_batch(variants, reads, ref, overhang=25, host=True, **kw)
    assert [x for x in got[1] if x[0] == 1][0][1] == 1
