"""Polyphase read scoring on the device: ``whatshap.polyphase.solver`` (whatshap/polyphase/solver.pyx:27-142) for the first phase of
``whatshap polyphase`` -- ``AlleleMatrix``, ``TriangleSparseMatrix`` and ``scoreReadset`` (src/polyphase/readscoring.cpp:17-84).

The matrices, genotype likelihoods and the per-position term tables are computed on the host inside the native library, the pair loop on
the device; ``host=True`` runs the pair loop of the debug library on the host instead (test infrastructure, bit-identical to the device).
A position's genotypes are summed in the order of the reference's unordered_map (as GNU libstdc++ iterates it; csrc/polyscore.cpp): the
stored set, scores, NaN count and estimated error rate equal the reference's on every recorded case.  There is no CPU fallback: without a device the native library raises.
"""

from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native

_UNDEFINED = 0xFFFFFFFF   # getFirstPos of an empty read


class AlleleMatrix:
    """AlleleMatrix (src/polyphase/allelematrix.cpp): reads as rows of (local position, allele), positions as sorted global positions.

    Built from our ``core.ReadSet``, from WhatsHap's ``ReadSet`` (through the compiled ingestion when it is loaded, else through the
    Python API), or from CSR arrays with :meth:`from_csr`.  As ``AlleleMatrix(ReadSet*)`` does: a read's first / last position is the
    local index of its first / last LISTED variant, a position listed twice keeps the allele listed last and counts twice in the depths.
    """

    def __init__(self, readset=None):
        if readset is None:
            self._set_csr(np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int8))
            return
        read_ptr, pos, alle = _flatten(readset)
        self._set_csr(read_ptr, pos, alle)

    @classmethod
    def from_csr(cls, read_ptr, positions, alleles) -> "AlleleMatrix":
        am = cls.__new__(cls)
        am._set_csr(np.asarray(read_ptr, dtype=np.uint64), np.asarray(positions, dtype=np.int64), np.asarray(alleles, dtype=np.int64))
        return am

    def _set_csr(self, read_ptr, pos, alle):
        alle = np.asarray(alle)
        if alle.size and (alle.min() < 0):
            raise ValueError(f"negative allele {int(alle.min())}: the reference's AlleleMatrix is undefined on it")
        if alle.size and alle.max() > 15:
            raise ValueError(f"allele {int(alle.max())} above 15: the reference's Genotype holds at most 16 alleles")
        pos = np.asarray(pos, dtype=np.int64)
        if pos.size and (pos.min() < 0 or pos.max() > 0xFFFFFFFF):
            raise ValueError("position outside [0, 2^32)")
        self.read_ptr = np.ascontiguousarray(read_ptr, dtype=np.uint64)
        self.position = np.ascontiguousarray(pos)
        self.allele = np.ascontiguousarray(alle, dtype=np.int8)
        self._derived = None

    # ---- the native view
    def view(self) -> _native.PolyMatrixView:
        return _native.PolyMatrixView(len(self), _native._ptr(self.read_ptr, C.c_uint64), _native._ptr(self.position, C.c_int64),
                                      _native._ptr(self.allele, C.c_int8))

    # ---- getters (computed once, in numpy)
    def _d(self):
        if self._derived is not None:
            return self._derived
        n = len(self)
        positions, local = np.unique(self.position, return_inverse=True)
        local = local.astype(np.int64).reshape(-1)
        read_of = np.repeat(np.arange(n, dtype=np.int64), np.diff(self.read_ptr.astype(np.int64)))
        max_allele = int(self.allele.max()) + 1 if self.allele.size else 0
        depths = np.zeros((len(positions), max_allele), dtype=np.int64)
        np.add.at(depths, (local, self.allele.astype(np.int64)), 1)
        starts, ends = self.read_ptr[:-1].astype(np.int64), self.read_ptr[1:].astype(np.int64)
        nonempty = ends > starts
        first = np.full(n, _UNDEFINED, dtype=np.int64)
        last = np.zeros(n, dtype=np.int64)
        first[nonempty] = local[starts[nonempty]]
        last[nonempty] = local[ends[nonempty] - 1]
        # rows sorted by local position, the allele listed last wins
        idx = np.arange(len(local), dtype=np.int64)
        o = np.lexsort((idx, local, read_of))
        r_s, p_s = read_of[o], local[o]
        keep = np.ones(len(o), dtype=bool)
        if len(o):
            keep[:-1] = (r_s[1:] != r_s[:-1]) | (p_s[1:] != p_s[:-1])
        o = o[keep]
        row_ptr = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.bincount(read_of[o], minlength=n), out=row_ptr[1:])
        self._derived = (positions, depths, first, last, row_ptr, local[o], self.allele[o].astype(np.int64), max_allele)
        return self._derived

    def __len__(self) -> int:
        return len(self.read_ptr) - 1

    def __iter__(self):
        return (self.getRead(i) for i in range(len(self)))

    def getNumPositions(self) -> int:
        return len(self._d()[0])

    def getPositions(self) -> List[int]:
        return [int(p) for p in self._d()[0]]

    def getMaxNumAllele(self) -> int:
        return self._d()[7]

    def getAlleleDepths(self, position: int) -> List[int]:
        return [int(x) for x in self._d()[1][position]]

    def getRead(self, read_id: int) -> List[Tuple[int, int]]:
        _, _, _, _, row_ptr, pos, alle, _ = self._d()
        b, e = row_ptr[read_id], row_ptr[read_id + 1]
        return [(int(p), int(a)) for p, a in zip(pos[b:e], alle[b:e])]

    def getFirstPos(self, read_id: int) -> int:
        return int(self._d()[2][read_id])

    def getLastPos(self, read_id: int) -> int:
        return int(self._d()[3][read_id])

    def getGlobalId(self, read_id: int) -> int:
        return read_id


def _flatten(readset) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(read_ptr, positions, alleles) of our ReadSet mirror or of WhatsHap's ReadSet."""
    from . import core

    if isinstance(readset, core.ReadSet):
        reads = list(readset)
        lens = np.fromiter((len(r) for r in reads), dtype=np.uint64, count=len(reads))
        read_ptr = np.zeros(len(reads) + 1, dtype=np.uint64)
        np.cumsum(lens, out=read_ptr[1:])
        pos = np.fromiter((p for r in reads for p in r._positions), dtype=np.int64, count=int(read_ptr[-1]))
        alle = np.fromiter((a for r in reads for a in r._alleles), dtype=np.int64, count=int(read_ptr[-1]))
        return read_ptr, pos, alle
    from . import ingest

    compiled = ingest.load()
    if compiled is not None:
        try:
            read_ptr, pos, alle, _qual, _samples = compiled.flatten_readset(readset)
            return np.asarray(read_ptr, dtype=np.uint64), np.asarray(pos, dtype=np.int64), np.asarray(alle, dtype=np.int64)
        except TypeError:
            pass
    read_ptr, pos, alle = [0], [], []
    for read in readset:
        for v in read:
            pos.append(v.position)
            alle.append(v.allele)
        read_ptr.append(len(pos))
    return np.asarray(read_ptr, dtype=np.uint64), np.asarray(pos, dtype=np.int64), np.asarray(alle, dtype=np.int64)


class TriangleSparseMatrix:
    """TriangleSparseMatrix (src/polyphase/trianglesparsematrix.cpp): float scores of unordered pairs (i != j), 0 where unset.
    ``getEntries`` returns the pairs (i, j), i > j, in increasing triangular index i*(i-1)/2 + j (the reference's returns them in hash
    order; its ``getIndices`` is sorted the same way)."""

    def __init__(self, i=None, j=None, score=None):
        self._m = {}
        self._arrays = None
        if i is not None:
            self._arrays = (np.asarray(i, dtype=np.uint32), np.asarray(j, dtype=np.uint32), np.asarray(score, dtype=np.float32))

    def _dict(self):
        if self._arrays is not None:
            i, j, s = self._arrays
            self._m = dict(zip(zip(i.tolist(), j.tolist()), s.tolist()))
            self._arrays = None
        return self._m

    @staticmethod
    def _key(i: int, j: int):
        return (i, j) if i > j else (j, i)

    def set(self, i: int, j: int, v: float) -> None:
        if i == j:
            return
        self._dict()[self._key(i, j)] = float(np.float32(v))

    def get(self, i: int, j: int) -> float:
        if i == j:
            return 0.0
        return self._dict().get(self._key(i, j), 0.0)

    def size(self) -> int:
        return len(self)

    def __len__(self) -> int:
        return len(self._arrays[0]) if self._arrays is not None else len(self._m)

    def getEntries(self) -> List[Tuple[int, int]]:
        i, j, _ = self.arrays()
        return list(zip(i.tolist(), j.tolist()))

    def __iter__(self):
        return iter(self.getEntries())

    def arrays(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(i, j, score) as numpy arrays, i > j, in triangular order."""
        if self._arrays is not None:
            return self._arrays
        if not self._m:
            return np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.float32)
        keys = np.array(list(self._m.keys()), dtype=np.uint64)
        vals = np.array(list(self._m.values()), dtype=np.float32)
        o = np.lexsort((keys[:, 1], keys[:, 0]))
        return keys[o, 0].astype(np.uint32), keys[o, 1].astype(np.uint32), vals[o]


def score_readsets_batch(matrices: Sequence[AlleleMatrix], minOverlap: int, ploidy: int, err: float = 0.0, device: int = 0, host: bool = False,
                         stats: Optional[list] = None) -> List[TriangleSparseMatrix]:
    """scoreReadset for every matrix, in one native call (one launch sequence for the whole batch).  ``stats``, if given, receives one
    dict per matrix (err used, counts, and the timings of the whole call)."""
    with _native.batch_handle(host, [am.view() for am in matrices], "whamd_poly_score", "whamd_debug_poly_score_host", "whamd_poly_score_destroy",
                              int(minOverlap), int(ploidy), float(err), device=device) as (L, h):
        out = []
        for k in range(len(matrices)):
            cnt = L.whamd_poly_score_count(h, k)
            i = np.empty(cnt, dtype=np.uint32)
            j = np.empty(cnt, dtype=np.uint32)
            s = np.empty(cnt, dtype=np.float32)
            if cnt:
                _native.checked(L, L.whamd_poly_score_get(h, k, _native._ptr(i, C.c_uint32), _native._ptr(j, C.c_uint32), _native._ptr(s, C.c_float)))
            out.append(TriangleSparseMatrix(i, j, s))
            if stats is not None:
                stats.append(_native.read_stats(L, "whamd_poly_score_get_stats", _native.PolyScoreStats, h, k))
        return out


def scoreReadset(am: AlleleMatrix, minOverlap: int, ploidy: int, err: float = 0.0, device: int = 0, host: bool = False,
                 stats: Optional[dict] = None) -> TriangleSparseMatrix:
    """whatshap.polyphase.solver.scoreReadset (solver.pyx:134-142)."""
    st: list = []
    result = score_readsets_batch([am], minOverlap, ploidy, err, device=device, host=host, stats=st)[0]
    if stats is not None:
        stats.update(st[0])
    return result


class ReadScoring:
    """whatshap.polyphase.solver.ReadScoring (solver.pyx:120-131)."""

    def scoreReadset(self, am: AlleleMatrix, minOverlap: int, ploidy: int, err: float = 0.0, device: int = 0, host: bool = False) -> TriangleSparseMatrix:
        return scoreReadset(am, minOverlap, ploidy, err, device=device, host=host)


def estimate_allele_error_rate(am: AlleleMatrix, ploidy: int, device: int = 0, host: bool = False) -> float:
    """ReadScoring::estimateAlleleErrorRate (readscoring.cpp:86-107), without its printing.  Host work in either library (``device``
    is accepted for symmetry with the other calls)."""
    L = _native.debug_lib() if host else _native.lib()
    v = am.view()
    out = C.c_double()
    _native.checked(L, L.whamd_poly_estimate_error_rate(C.byref(v), int(ploidy), C.byref(out)))
    return out.value
