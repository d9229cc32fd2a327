"""CPU: polyphase read scoring, host side.  The debug library's restatement (matrices, genotype likelihoods, term tables and windows of
csrc/polyscore.cpp, then the pair loop on one host thread, the device's bit-exact reference) against every recorded result of the
reference's ReadScoring::scoreReadset (tests/golden/make_polyphase_golden.py); the AlleleMatrix getters against the recorded ones;
duplicate positions, negative-allele refusal and TriangleSparseMatrix semantics."""
import ctypes as C

import numpy as np
import pytest

from polyphase_cases import expected, load, matrix, ulp_distance
from whatshap_amd import _native, core, polyphase

CASES = load()
# Scores may differ from the reference's by one float ulp where its unordered_map sums a position's genotypes in another order;
# this many entries of the recorded set do (the rest are bit-identical).
MAX_ULP_DIFFERENCES = 0


def check_case(case, got, stats):
    ei, ej, es = expected(case)
    i, j, s = got.arrays()
    assert np.array_equal(i, ei) and np.array_equal(j, ej), case["kind"]
    d = ulp_distance(s, es)
    assert d.max(initial=0) <= 1, case["kind"]
    assert stats["n_nan"] == case["nans"]
    if case["ploidy"] >= 2:
        assert stats["err"] == case["err_used"]
    return int((d != 0).sum())


def test_host_equals_reference_on_every_case():
    differing = 0
    for case in CASES:
        st = {}
        got = polyphase.scoreReadset(matrix(case), case["min_overlap"], case["ploidy"], case["err"], host=True, stats=st)
        differing += check_case(case, got, st)
        assert st["launches"] == 0
    assert differing <= MAX_ULP_DIFFERENCES


def test_host_batch_equals_one_by_one():
    ms = [matrix(c) for c in CASES[:60]]
    for mo, ploidy, err in ((1, 3, 0.07), (2, 4, 0.0)):
        batch = polyphase.score_readsets_batch(ms, mo, ploidy, err, host=True)
        for m, b in zip(ms, batch):
            one = polyphase.scoreReadset(m, mo, ploidy, err, host=True)
            for x, y in zip(b.arrays(), one.arrays()):
                assert np.array_equal(x, y)


def test_estimated_error_rate_equals_reference():
    for case in CASES:
        if case["err"] == 0.0 and case["ploidy"] >= 2:
            assert polyphase.estimate_allele_error_rate(matrix(case), case["ploidy"], host=True) == case["err_used"]


@pytest.mark.parametrize("k", [k for k, c in enumerate(CASES) if "getters" in c][::7])
def test_allele_matrix_getters_equal_reference(k):
    case = CASES[k]
    g = case["getters"]
    am = matrix(case)
    assert len(am) == len(case["reads"])
    assert am.getPositions() == g["positions"]
    assert am.getNumPositions() == len(g["positions"])
    assert [am.getFirstPos(r) for r in range(len(am))] == g["first"]
    assert [am.getLastPos(r) for r in range(len(am))] == g["last"]
    assert am.getMaxNumAllele() == g["maxallele"]
    depths = [d for p in range(am.getNumPositions()) for d in am.getAlleleDepths(p)]
    assert depths == g["depths"]
    assert [[list(e) for e in am.getRead(r)] for r in range(len(am))] == g["rows"]
    assert [am.getGlobalId(r) for r in range(len(am))] == list(range(len(am)))


def test_duplicate_positions_keep_last_allele_and_count_twice():
    am = polyphase.AlleleMatrix.from_csr([0, 3, 5], [10, 20, 20, 20, 30], [0, 1, 0, 1, 1])
    assert am.getRead(0) == [(0, 0), (1, 0)]
    assert am.getAlleleDepths(1) == [1, 2]
    assert any(c["kind"] == "duplicates" for c in CASES)


def test_from_our_readset_equals_csr():
    rs = core.ReadSet()
    for name, variants in (("a", [(10, 0), (20, 1), (30, 2)]), ("b", [(20, 1), (30, 2), (40, 0)]), ("c", [(30, 0), (40, 1)])):
        r = core.Read(name, 50, 0, 0)
        for p, a in variants:
            r.add_variant(p, a, 30)
        rs.add(r)
    am = polyphase.AlleleMatrix(rs)
    assert am.getPositions() == [10, 20, 30, 40]
    assert am.getRead(1) == [(1, 1), (2, 2), (3, 0)]
    a = polyphase.scoreReadset(am, 1, 3, 0.07, host=True).arrays()
    b = polyphase.scoreReadset(polyphase.AlleleMatrix.from_csr(am.read_ptr, am.position, am.allele), 1, 3, 0.07, host=True).arrays()
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert len(a[0]) >= 1


def test_negative_allele_refused():
    with pytest.raises(ValueError, match="negative allele"):
        polyphase.AlleleMatrix.from_csr([0, 2], [10, 20], [0, -1])
    # the native check, past the Python one
    ptr = np.array([0, 2], dtype=np.uint64)
    pos = np.array([10, 20], dtype=np.int64)
    alle = np.array([0, -1], dtype=np.int8)
    view = _native.PolyMatrixView(1, _native._ptr(ptr, C.c_uint64), _native._ptr(pos, C.c_int64), _native._ptr(alle, C.c_int8))
    L = _native.debug_lib()
    h = C.c_void_p()
    assert L.whamd_debug_poly_score_host(C.byref(view), 1, 1, 2, 0.07, C.byref(h)) == _native.WHAMD_ERR_INVALID
    assert b"negative allele" in L.whamd_last_error()


def test_ploidy_above_15_refused():
    am = polyphase.AlleleMatrix.from_csr([0, 2, 4], [10, 20, 10, 20], [0, 1, 0, 1])
    with pytest.raises(ValueError, match="above 15"):
        polyphase.scoreReadset(am, 1, 16, 0.07, host=True)


def test_empty_reads_and_ploidy_below_2():
    pos, alle = [10, 20, 30, 10, 20, 20, 30], [0, 1, 1, 1, 1, 0, 1]
    am = polyphase.AlleleMatrix.from_csr([0, 3, 3, 5, 5, 7], pos, alle)   # reads 1 and 3 are empty
    assert am.getFirstPos(1) == 0xFFFFFFFF and am.getLastPos(1) == 0
    dense = polyphase.AlleleMatrix.from_csr([0, 3, 5, 7], pos, alle)
    ids = np.array([0, 2, 4], dtype=np.uint32)
    for mo in (0, 1, 2, 3):
        i, j, s = polyphase.scoreReadset(am, mo, 2, 0.07, host=True).arrays()
        di, dj, ds = polyphase.scoreReadset(dense, mo, 2, 0.07, host=True).arrays()
        assert np.array_equal(i, ids[di]) and np.array_equal(j, ids[dj]) and np.array_equal(s, ds)
    assert len(polyphase.scoreReadset(dense, 1, 2, 0.07, host=True)) > 0
    for ploidy in (0, 1):
        st = {}
        assert len(polyphase.scoreReadset(am, 1, ploidy, 0.07, host=True, stats=st)) == 0
        assert st["n_candidates"] == 0


def test_triangle_sparse_matrix_semantics():
    m = polyphase.TriangleSparseMatrix()
    m.set(3, 3, 1.0)
    assert len(m) == 0 and m.get(3, 3) == 0.0
    m.set(2, 5, 0.1)
    m.set(4, 1, -2.5)
    m.set(5, 0, 7.0)
    assert m.get(5, 2) == m.get(2, 5) == float(np.float32(0.1))
    assert m.get(0, 1) == 0.0
    assert m.size() == len(m) == 3
    assert m.getEntries() == [(4, 1), (5, 0), (5, 2)]   # increasing triangular index i*(i-1)/2 + j
    assert list(m) == m.getEntries()
    i, j, s = m.arrays()
    assert i.tolist() == [4, 5, 5] and j.tolist() == [1, 0, 2] and s.dtype == np.float32
    m.set(1, 4, 3.0)
    assert m.get(4, 1) == 3.0 and len(m) == 3
