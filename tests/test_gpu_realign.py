"""GPU: allele detection by re-alignment on the MI355X (csrc/realign_device.hip) against the reference's recorded yields and distances,
a plain Python restatement on random pairs (multi-word Myers, multi-strip Gotoh), and the debug library's host path on a batch of more
than a million jobs."""
import random

import numpy as np
import pytest

from realign_cases import affine_distance, group_objects, load, unit_distance
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
