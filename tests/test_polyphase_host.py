"""CPU: polyphase read scoring, host side.  The debug library's restatement (matrices, genotype likelihoods, term tables and windows of
csrc/polyscore.cpp, then the pair loop on one host thread, the device's bit-exact reference) against every recorded result of the
reference's ReadScoring::scoreReadset (tests/golden/make_polyphase_golden.py), the second recording of NaN scores, ploidy up to 15,
16 alleles, far-apart positions and long shared stretches included; the AlleleMatrix getters against the recorded ones; duplicate
positions, the refusals (negative allele, allele above 15, position outside [0, 2^32), ploidy above 15) and TriangleSparseMatrix
semantics."""
import ctypes as C

import numpy as np
import pytest

from polyphase_cases import BITMAP_SLACK, EDGE_KINDS, expected, load, load_edge, matrix, span_and_entries, takes_sort_branch, ulp_distance
from whatshap_amd import _native, core, polyphase

CASES = load()
# Scores may differ from the reference's by one float ulp where its unordered_map sums a position's genotypes in another order than
# hash_order (csrc/polyscore.cpp) restates; this many entries of the recorded set do (the rest are bit-identical).
MAX_ULP_DIFFERENCES = 0
EDGE = load_edge()
# The same count over the second recording, of every kind (nan, high_ploidy, many_alleles, sparse_positions, long_overlap): none, the
# sums of thousands of terms of long_overlap included.
EDGE_ULP_DIFFERENCES = 0


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


@pytest.mark.parametrize("kind", EDGE_KINDS)
def test_host_equals_reference_on_edge_cases(kind):
    """Two many_alleles cases (ploidy 3 with 16 alleles, ploidy 4 with 8, err = 0.2) are why csrc/polyscore.cpp sums a position's
    genotypes in the reference's hash order: at a position with exactly six alleles present 1 - err * (n_ex - 1) is 0.0 and same / diff
    of two different alleles is 1 but for rounding, so the term is 0.0 or 1e-16 by the order of the sum, and a pair whose terms are
    all 0.0 is not stored.  Summed in increasing genotype index, 12 pairs were stored on one side only."""
    differing = 0
    for case in (c for c in EDGE if c["kind"] == kind):
        st = {}
        got = polyphase.scoreReadset(matrix(case), case["min_overlap"], case["ploidy"], case["err"], host=True, stats=st)
        differing += check_case(case, got, st)
        assert st["launches"] == 0
    assert differing == EDGE_ULP_DIFFERENCES


def test_edge_recording_covers_what_it_exists_for():
    nan = [c for c in EDGE if c["nans"] > 0]
    assert len(nan) >= 3 and any(c["expected"]["i"] for c in nan)          # NaN pairs, and NaN next to stored pairs
    assert all(c["nans"] > 0 for c in EDGE if c["kind"] == "nan")
    assert any(c["getters"]["maxallele"] == 16 for c in EDGE if "getters" in c)
    assert any(a == 15 for c in EDGE if c["kind"] == "many_alleles" for r in c["reads"] for _, a in r)
    present = {(c["err"], sum(d > 0 for d in c["getters"]["depths"][p * A:(p + 1) * A]))
               for c in EDGE if c["kind"] == "many_alleles" for A in [c["getters"]["maxallele"]] for p in range(len(c["getters"]["positions"]))}
    assert {(0.2, 5), (0.2, 6), (0.2, 7)} <= present                        # 1 - err * (n_ex - 1): 0.2, 0.0, negative
    assert {c["ploidy"] for c in EDGE if c["kind"] == "high_ploidy"} == {7, 8, 10, 12, 15}
    assert sum(takes_sort_branch(c) for c in EDGE) >= 5                      # poly_build_matrix's sort-and-search branch ...
    at = [span_and_entries(c) for c in EDGE if c["kind"] == "sparse_positions" and not takes_sort_branch(c)]
    assert at and all(span == 64 * n + BITMAP_SLACK for span, n in at)      # ... and the largest span of its bitmap branch
    assert any(span == 64 * n + BITMAP_SLACK + 1 for span, n in map(span_and_entries, EDGE))
    assert max(p for c in EDGE for r in c["reads"] for p, _ in r) == 2**31 - 1
    assert max(len(r) for c in EDGE for r in c["reads"]) >= 2000
    assert any(c["min_overlap"] >= 100 and c["expected"]["i"] for c in EDGE if c["kind"] == "long_overlap")


def test_host_batch_equals_one_by_one():
    ms = [matrix(c) for c in CASES[:60]]
    for mo, ploidy, err in ((1, 3, 0.07), (2, 4, 0.0)):
        batch = polyphase.score_readsets_batch(ms, mo, ploidy, err, host=True)
        for m, b in zip(ms, batch):
            one = polyphase.scoreReadset(m, mo, ploidy, err, host=True)
            for x, y in zip(b.arrays(), one.arrays()):
                assert np.array_equal(x, y)


def test_estimated_error_rate_equals_reference():
    for case in CASES + EDGE:
        if case["err"] == 0.0 and case["ploidy"] >= 2:
            assert polyphase.estimate_allele_error_rate(matrix(case), case["ploidy"], host=True) == case["err_used"]


@pytest.mark.parametrize("k", [k for k, c in enumerate(CASES) if "getters" in c][::7])
def test_allele_matrix_getters_equal_reference(k):
    check_getters(CASES[k])


@pytest.mark.parametrize("kind", [k for k in EDGE_KINDS if k != "long_overlap"])   # (long_overlap records no getters: its size)
def test_allele_matrix_getters_equal_reference_on_edge_cases(kind):
    cases = [c for c in EDGE if c["kind"] == kind]
    assert all("getters" in c for c in cases)
    for case in cases:
        check_getters(case)


def check_getters(case):
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


def native_status(pos, alle):
    ptr = np.array([0, len(pos)], dtype=np.uint64)
    pos = np.array(pos, dtype=np.int64)
    alle = np.array(alle, dtype=np.int8)
    view = _native.PolyMatrixView(1, _native._ptr(ptr, C.c_uint64), _native._ptr(pos, C.c_int64), _native._ptr(alle, C.c_int8))
    L = _native.debug_lib()
    h = C.c_void_p()
    return L.whamd_debug_poly_score_host(C.byref(view), 1, 1, 2, 0.07, C.byref(h)), L.whamd_last_error()


def test_allele_above_15_refused():
    assert len(polyphase.AlleleMatrix.from_csr([0, 2], [10, 20], [0, 15])) == 1
    with pytest.raises(ValueError, match="allele 16 above 15"):
        polyphase.AlleleMatrix.from_csr([0, 2], [10, 20], [0, 16])
    status, message = native_status([10, 20], [0, 16])   # the native check, past the Python one
    assert status == _native.WHAMD_ERR_INVALID and b"allele 16 above 15" in message


def test_position_outside_uint32_refused():
    assert polyphase.AlleleMatrix.from_csr([0, 2], [0, 2**32 - 1], [0, 1]).getPositions() == [0, 2**32 - 1]
    for pos in ([-1, 20], [10, 2**32]):
        with pytest.raises(ValueError, match="position outside"):
            polyphase.AlleleMatrix.from_csr([0, 2], pos, [0, 1])
        status, message = native_status(pos, [0, 1])
        assert status == _native.WHAMD_ERR_INVALID and b"position outside" in message
    # both ends of the range are scored, on either side of poly_build_matrix's choice between bitmap and sort
    for pos in ([0, 5, 2**32 - 1], [2**32 - 9, 2**32 - 5, 2**32 - 1]):
        am = polyphase.AlleleMatrix.from_csr([0, 3, 6], pos + pos, [0, 1, 1, 0, 1, 0])
        near = polyphase.AlleleMatrix.from_csr([0, 3, 6], [1, 2, 3, 1, 2, 3], [0, 1, 1, 0, 1, 0])
        a, b = (polyphase.scoreReadset(m, 2, 2, 0.07, host=True).arrays() for m in (am, near))
        assert len(a[0]) == 1 and all(np.array_equal(x, y) for x, y in zip(a, b))


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
