"""GPU: polyphase read scoring on the device.  Against every recorded result of the reference (tests/golden/make_polyphase_golden.py),
bit-identical to the host pair loop of the debug library on large random blocks (50 000 long-read-like reads with windows of hundreds
of partners and anchors spanning 20 000 variants), a batch of 500 blocks against the same blocks one by one, and the calls that need
no device work."""
import numpy as np
import pytest

from polyphase_cases import expected, load, matrix, random_block, ulp_distance
from whatshap_amd import polyphase

pytestmark = pytest.mark.gpu

CASES = load()


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a.arrays(), b.arrays()))


def check(case, got, stats):
    ei, ej, es = expected(case)
    i, j, s = got.arrays()
    assert np.array_equal(i, ei) and np.array_equal(j, ej), case["kind"]
    assert ulp_distance(s, es).max(initial=0) <= 1
    assert stats["n_nan"] == case["nans"]
    if case["ploidy"] >= 2:
        assert stats["err"] == case["err_used"]


def test_device_equals_reference_case_by_case():
    for case in CASES:
        st = {}
        got = polyphase.scoreReadset(matrix(case), case["min_overlap"], case["ploidy"], case["err"], stats=st)
        check(case, got, st)
        host = polyphase.scoreReadset(matrix(case), case["min_overlap"], case["ploidy"], case["err"], host=True)
        assert same(got, host)


def test_device_equals_reference_as_batches():
    groups = {}
    for case in CASES:
        groups.setdefault((case["min_overlap"], case["ploidy"], case["err"]), []).append(case)
    for (mo, ploidy, err), cases in groups.items():
        stats = []
        got = polyphase.score_readsets_batch([matrix(c) for c in cases], mo, ploidy, err, stats=stats)
        for case, g, st in zip(cases, got, stats):
            check(case, g, st)


# (three alleles at ploidy 6 with err = 0 would test little: the reference's estimate is then 0.0 -- every depth sum is NaN or -inf,
# none beats the initial -inf -- and every term is 0 or NaN)
@pytest.mark.parametrize("seed,ploidy,n_alleles,min_overlap,err", [(1, 4, 2, 2, 0.07), (2, 6, 2, 1, 0.0), (3, 3, 3, 1, 0.07)])
def test_device_bit_identical_to_host_on_large_block(seed, ploidy, n_alleles, min_overlap, err):
    ptr, pos, alle = random_block(seed, 50_000, 40_000, ploidy=ploidy, n_alleles=n_alleles, min_len=20, max_len=300,
                                  long_every=2_500, long_len=20_000)
    am = polyphase.AlleleMatrix.from_csr(ptr, pos, alle)
    dev_st, host_st = {}, {}
    dev = polyphase.scoreReadset(am, min_overlap, ploidy, err, stats=dev_st)
    host = polyphase.scoreReadset(am, min_overlap, ploidy, err, host=True, stats=host_st)
    assert dev_st["n_candidates"] > 50_000 * 100          # windows of hundreds
    assert dev_st["n_entries"] > 1_000_000
    assert same(dev, host)
    for k in ("err", "n_candidates", "n_overlapping", "n_entries", "n_nan", "n_pair_positions"):
        assert dev_st[k] == host_st[k], k
    assert dev_st["launches"] > 0


def test_batch_of_500_blocks_equals_one_by_one():
    blocks = [polyphase.AlleleMatrix.from_csr(*random_block(100 + b, 20 + b % 60, 80, ploidy=4, n_alleles=2 + b % 3, min_len=2, max_len=25))
              for b in range(500)]
    blocks[7] = polyphase.AlleleMatrix()   # an empty block inside the batch
    stats = []
    batch = polyphase.score_readsets_batch(blocks, 2, 4, 0.0, stats=stats)
    assert len(batch) == 500
    assert stats[0]["launches"] == 4       # one launch sequence for all of them
    for m, b, st in zip(blocks, batch, stats):
        one_st = {}
        one = polyphase.scoreReadset(m, 2, 4, 0.0, stats=one_st)
        assert same(b, one)
        assert st["n_entries"] == one_st["n_entries"] and st["err"] == one_st["err"]


def test_edge_cases_return_without_launch():
    disjoint = polyphase.AlleleMatrix.from_csr([0, 2, 4, 6], [10, 11, 20, 21, 30, 31], [0, 1, 1, 0, 0, 1])
    some = polyphase.AlleleMatrix.from_csr([0, 2, 4], [10, 20, 10, 20], [0, 1, 1, 1])
    for am, mo, ploidy in ((polyphase.AlleleMatrix(), 1, 4), (some, 1, 1), (some, 1, 0), (disjoint, 1, 2), (disjoint, 2, 3)):
        st = {}
        assert len(polyphase.scoreReadset(am, mo, ploidy, 0.07, stats=st)) == 0
        assert st["launches"] == 0 and st["kernel_ms"] == 0.0
    # minOverlap 3 on the first read, whose last local position is 1: the reference's uint32 terminal wraps, every later read is a
    # candidate (and shares too little to be stored)
    st = {}
    assert len(polyphase.scoreReadset(disjoint, 3, 3, 0.07, stats=st)) == 0
    assert st["n_candidates"] == 2 and st["n_overlapping"] == 0
    assert st["launches"] == 2 and st["download_ms"] == 0.0   # pair kernel and scan; nothing kept, so no compaction, sort or download
    stats = []
    assert polyphase.score_readsets_batch([], 1, 2, 0.07, stats=stats) == []
