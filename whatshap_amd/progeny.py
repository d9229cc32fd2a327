"""Progeny marker scoring on the device: the "scoring" stage of ``whatshap polyphasegenetic`` -- ``get_variant_scoring``,
``get_most_likely_variant_type`` and ``compute_gt_likelihood_priors`` of whatshap/polyphase/offspringscoring.py and the
``ProgenyGenotypeLikelihoods`` class of whatshap/polyphase/solver.pyx:233-270 (src/polyphase/progenygenotypelikelihoods.cpp).

The native library finds the stored entries on the host and scores them with one device lane per entry; ``host=True`` runs the same
inner function on one host thread of the debug library instead (test infrastructure: bit-identical to the reference).  Device scores
differ from the reference's only through ``log`` (device math library against the host's).  There is no CPU fallback: without a device
the native library raises.
"""

from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native
from .polyphase import TriangleSparseMatrix, _raise

_KIND_SN, _KIND_S2, _KIND_DN = 0, 1, 2


class ProgenyGenotypeLikelihoods:
    """ProgenyGenotypeLikelihoods (solver.pyx:233-270): genotype likelihoods [position][sample][genotype 0 .. ploidy], kept as float32
    (the reference's table is ``std::vector<float>``: values are rounded when set and widened when read), ``-1`` = no data.

    As in the reference, ``numPositions`` is fixed by the constructor: setting a row at or beyond it neither fails nor becomes visible
    (``getGl`` returns 0.0 there, ``getGlv`` zeros), and scores treat such a row as zeros."""

    def __init__(self, ploidy: int, numSamples: int, numPositions: int):
        if ploidy < 0 or numSamples < 0 or numPositions < 0:
            raise OverflowError("can't convert negative value to uint32_t")
        if (numPositions + 1) * numSamples * (ploidy + 1) >= 1 << 32:
            raise ValueError("(numPositions + 1) * numSamples * (ploidy + 1) reaches 2^32: the reference's uint32 index would wrap")
        self._ploidy, self._n_samples, self._n_positions = int(ploidy), int(numSamples), int(numPositions)
        self._gl = np.full((self._n_positions, self._n_samples, self._ploidy + 1), -1.0, dtype=np.float32)

    @classmethod
    def from_array(cls, a) -> "ProgenyGenotypeLikelihoods":
        """A table from an array [numPositions][numSamples][ploidy + 1] (rounded to float32; not copied if it already is C-contiguous float32)."""
        a = np.asarray(a)
        if a.ndim != 3 or a.shape[2] < 1:
            raise ValueError("expected an array [numPositions][numSamples][ploidy + 1]")
        t = cls.__new__(cls)
        t._n_positions, t._n_samples, t._ploidy = a.shape[0], a.shape[1], a.shape[2] - 1
        if (t._n_positions + 1) * t._n_samples * (t._ploidy + 1) >= 1 << 32:
            raise ValueError("(numPositions + 1) * numSamples * (ploidy + 1) reaches 2^32: the reference's uint32 index would wrap")
        t._gl = np.ascontiguousarray(a, dtype=np.float32)
        return t

    def array(self) -> np.ndarray:
        """The visible table, float32 [numPositions][numSamples][ploidy + 1]."""
        return self._gl

    def getPloidy(self) -> int:
        return self._ploidy

    def getNumSamples(self) -> int:
        return self._n_samples

    def getNumPositions(self) -> int:
        return self._n_positions

    def __len__(self) -> int:
        return self._n_positions

    def getGl(self, pos: int, sample_id: int, genotype: int) -> float:
        if pos >= self._n_positions:
            return 0.0
        return float(self._gl[pos, sample_id, genotype])

    def getGlv(self, pos: int, sample_id: int) -> List[float]:
        if pos >= self._n_positions:
            return [0.0] * (self._ploidy + 1)
        return [float(x) for x in self._gl[pos, sample_id]]

    def setGl(self, pos: int, sample_id: int, genotype: int, gl: float) -> None:
        if pos >= self._n_positions:
            return   # (the reference grows its vector but not numPositions: the value can never be read)
        self._gl[pos, sample_id, genotype] = gl

    def setGlv(self, pos: int, sample_id: int, gl: Sequence[float]) -> None:
        if pos >= self._n_positions:
            return
        self._gl[pos, sample_id, :] = np.asarray(gl[: self._ploidy + 1], dtype=np.float64)

    def _pair(self, pos1: int, pos2: int, kind: int) -> float:
        L = _native.debug_lib()
        out = C.c_double()
        st = L.whamd_debug_progeny_pair_score_host(_native._ptr(self._gl, C.c_float), self._n_positions, self._n_samples, self._ploidy, int(pos1),
                                                   int(pos2), kind, C.byref(out))
        if st != _native.WHAMD_OK:
            _raise(L, st)
        return out.value

    # the single-pair getters: host arithmetic (the debug library's twin of the device's inner function)
    def getSimplexNulliplexScore(self, pos1: int, pos2: int) -> float:
        return self._pair(pos1, pos2, _KIND_SN)

    def getSimplexSimplexScore(self, pos1: int, pos2: int) -> float:
        return self._pair(pos1, pos2, _KIND_S2)

    def getDuplexNulliplexScore(self, pos1: int, pos2: int) -> float:
        return self._pair(pos1, pos2, _KIND_DN)


class VariantScoring(TriangleSparseMatrix):
    """What :func:`get_variant_scoring` returns: the TriangleSparseMatrix of the stored float scores, plus the double scores they were
    rounded from (:meth:`scores_f64`, in the order of :meth:`arrays`)."""

    def __init__(self, i, j, score, score_f64):
        super().__init__(i, j, score)
        self._f64 = np.asarray(score_f64, dtype=np.float64)

    def scores_f64(self) -> np.ndarray:
        return self._f64


class ProgenyProblem:
    """One call's input: the table, node -> variant, the variants' (alt_count, co_alt_count), the scoring window."""

    def __init__(self, off_gl: ProgenyGenotypeLikelihoods, node_variant, alt_count, co_alt_count, scoring_window: int):
        self.off_gl = off_gl
        self.node_variant = np.ascontiguousarray(node_variant, dtype=np.uint32)
        self.alt_count = np.ascontiguousarray(alt_count, dtype=np.uint32)
        self.co_alt_count = np.ascontiguousarray(co_alt_count, dtype=np.uint32)
        if self.alt_count.shape != self.co_alt_count.shape:
            raise ValueError("alt_count and co_alt_count differ in length (mismatched lengths)")
        self.scoring_window = int(scoring_window)
        if self.scoring_window < 0 or self.scoring_window > 0xFFFFFFFF:
            raise ValueError("scoring_window must be at least 1")

    @classmethod
    def from_varinfo(cls, varinfo, off_gl: ProgenyGenotypeLikelihoods, phasing_param) -> "ProgenyProblem":
        """From the reference's objects, duck-typed: ``varinfo.get_node_positions()`` (the variant of every node),
        ``varinfo[v].alt_count`` / ``.co_alt_count``, ``phasing_param.scoring_window``."""
        nodes = np.asarray(list(varinfo.get_node_positions()), dtype=np.int64)
        if nodes.size and nodes.min() < 0:
            raise ValueError("negative variant id")
        n_variants = int(nodes.max()) + 1 if nodes.size else 0
        alt = np.zeros(n_variants, dtype=np.uint32)
        co = np.zeros(n_variants, dtype=np.uint32)
        for v in np.unique(nodes).tolist():
            alt[v] = varinfo[v].alt_count
            co[v] = varinfo[v].co_alt_count
        return cls(off_gl, nodes, alt, co, phasing_param.scoring_window)

    def view(self) -> _native.ProgenyView:
        t = self.off_gl
        return _native.ProgenyView(_native._ptr(t.array(), C.c_float), t.getNumPositions(), t.getNumSamples(), t.getPloidy(), self.node_variant.size,
                                   _native._ptr(self.node_variant, C.c_uint32), self.alt_count.size, _native._ptr(self.alt_count, C.c_uint32),
                                   _native._ptr(self.co_alt_count, C.c_uint32), self.scoring_window)


def score_variants_batch(problems: Sequence[ProgenyProblem], device: int = 0, host: bool = False, stats: Optional[list] = None) -> List[VariantScoring]:
    """get_variant_scoring for every problem in one native call (one upload, one launch, one download for the whole batch).  ``stats``,
    if given, receives one dict per problem (counts, and the timings of the whole call)."""
    L = _native.debug_lib() if host else _native.lib()
    n = len(problems)
    views = (_native.ProgenyView * max(n, 1))()
    for k, p in enumerate(problems):
        views[k] = p.view()
    h = C.c_void_p()
    if host:
        st = L.whamd_debug_progeny_score_host(views, n, C.byref(h))
    else:
        st = L.whamd_progeny_score(views, n, int(device), C.byref(h))
    if st != _native.WHAMD_OK:
        _raise(L, st)
    try:
        out = []
        for k in range(n):
            cnt = L.whamd_progeny_score_count(h, k)
            i = np.empty(cnt, dtype=np.uint32)
            j = np.empty(cnt, dtype=np.uint32)
            s32 = np.empty(cnt, dtype=np.float32)
            s64 = np.empty(cnt, dtype=np.float64)
            if cnt:
                st = L.whamd_progeny_score_get(h, k, _native._ptr(i, C.c_uint32), _native._ptr(j, C.c_uint32), _native._ptr(s32, C.c_float),
                                               _native._ptr(s64, C.c_double))
                if st != _native.WHAMD_OK:
                    _raise(L, st)
            out.append(VariantScoring(i, j, s32, s64))
            if stats is not None:
                ps = _native.ProgenyScoreStats()
                L.whamd_progeny_score_get_stats(h, k, C.byref(ps))
                stats.append(ps.as_dict())
        return out
    finally:
        L.whamd_progeny_score_destroy(h)


def get_variant_scoring(varinfo, off_gl: ProgenyGenotypeLikelihoods, phasing_param, device: int = 0, host: bool = False,
                        stats: Optional[dict] = None) -> VariantScoring:
    """whatshap.polyphase.offspringscoring.get_variant_scoring (offspringscoring.py:143-188)."""
    st: list = []
    result = score_variants_batch([ProgenyProblem.from_varinfo(varinfo, off_gl, phasing_param)], device=device, host=host, stats=st)[0]
    if stats is not None:
        stats.update(st[0])
    return result


def score_entries_host(problem: ProgenyProblem, i, j) -> Tuple[np.ndarray, np.ndarray]:
    """TEST INFRASTRUCTURE (debug library, one host thread): (stored, score) of the given pairs of one problem -- what the reference's
    loop stores for each of them, without scoring the whole problem."""
    L = _native.debug_lib()
    i = np.ascontiguousarray(i, dtype=np.uint32)
    j = np.ascontiguousarray(j, dtype=np.uint32)
    if i.shape != j.shape:
        raise ValueError("i and j differ in length")
    score = np.zeros(i.size, dtype=np.float64)
    stored = np.zeros(i.size, dtype=np.uint8)
    v = problem.view()
    st = L.whamd_debug_progeny_score_entries_host(C.byref(v), i.size, _native._ptr(i, C.c_uint32), _native._ptr(j, C.c_uint32),
                                                  _native._ptr(score, C.c_double), _native._ptr(stored, C.c_uint8))
    if st != _native.WHAMD_OK:
        _raise(L, st)
    return stored.astype(bool), score


def _hyp(k: int, N: int, M: int, n: int) -> float:
    # hyp (offspringscoring.py:33-34) with exact binomial coefficients: they are below 2^53 for every ploidy of practical use, where
    # scipy.special.binom returns the same doubles
    return float(math.comb(M, k)) * float(math.comb(N - M, n - k)) / float(math.comb(N, n)) if 0 <= k and 0 <= n - k else 0.0


def compute_gt_likelihood_priors(ploidy: int) -> List[List[List[float]]]:
    """compute_gt_likelihood_priors (offspringscoring.py:214-229): priors[i][j][l] = probability that a progeny inherits l alternative
    alleles when the parents carry i and j; same order of operations as the reference (Python's ``sum`` from 0)."""
    k = ploidy
    priors: List[List[List[float]]] = [[[] for _ in range(k + 1)] for _ in range(k + 1)]
    for i in range(k + 1):
        for j in range(i + 1):
            d = [sum([_hyp(l, k, i, k // 2) * _hyp(m - l, k, j, k // 2) for l in range(m + 1)]) for m in range(k + 1)]
            priors[i][j] = d
            priors[j][i] = d
    return priors


def most_likely_variant_types(priors, off_gl: ProgenyGenotypeLikelihoods, nodes=None, device: int = 0, host: bool = False):
    """get_most_likely_variant_type (offspringscoring.py:191-211) for the table rows ``nodes`` (default: every position): the list of
    winners ``(g0, g1)`` and the llh table [len(nodes)][(k+1)(k+2)/2] of all parental types in the reference's loop order."""
    L = _native.debug_lib() if host else _native.lib()
    k1 = off_gl.getPloidy() + 1
    pri = np.ascontiguousarray(priors, dtype=np.float64)
    if pri.shape != (k1, k1, k1):
        raise ValueError(f"priors must be [{k1}][{k1}][{k1}] for ploidy {k1 - 1} (mismatched lengths)")
    if nodes is None:
        nodes = np.arange(off_gl.getNumPositions(), dtype=np.uint32)
    nodes = np.ascontiguousarray(nodes, dtype=np.uint32)
    n_types = k1 * (k1 + 1) // 2
    llh = np.zeros((nodes.size, n_types), dtype=np.float64)
    g0 = np.zeros(nodes.size, dtype=np.uint32)
    g1 = np.zeros(nodes.size, dtype=np.uint32)
    args = [_native._ptr(off_gl.array(), C.c_float), off_gl.getNumPositions(), off_gl.getNumSamples(), off_gl.getPloidy(), _native._ptr(pri, C.c_double),
            _native._ptr(nodes, C.c_uint32), nodes.size]
    outs = [_native._ptr(llh, C.c_double), _native._ptr(g0, C.c_uint32), _native._ptr(g1, C.c_uint32)]
    if host:
        st = L.whamd_debug_progeny_variant_types_host(*args, *outs)
    else:
        st = L.whamd_progeny_variant_types(*args, int(device), *outs)
    if st != _native.WHAMD_OK:
        _raise(L, st)
    return list(zip(g0.tolist(), g1.tolist())), llh
