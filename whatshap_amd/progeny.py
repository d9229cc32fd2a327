"""Progeny marker scoring on the device: the "scoring" stage of ``whatshap polyphasegenetic`` -- ``get_offspring_gl`` /
``compute_gt_likelihoods``, ``correct_variant_types``, ``get_variant_scoring``, ``get_most_likely_variant_type`` and
``compute_gt_likelihood_priors`` of whatshap/polyphase/offspringscoring.py and the ``ProgenyGenotypeLikelihoods`` class of
whatshap/polyphase/solver.pyx:233-270 (src/polyphase/progenygenotypelikelihoods.cpp).

The table of genotype likelihoods is made from allele depths by one device lane per (sample, node) cell (:func:`offspring_gl_batch`), or
made and scored without leaving the device (:func:`score_variants_from_depths`).  Where the reference's ``binom.pmf`` values all underflow
(depths of a few hundred reads: ``ZeroDivisionError`` or NaN there) these return the correctly normalised likelihoods.

The native library finds the stored entries on the host and scores them with one device lane per entry; ``host=True`` runs the same
inner function on one host thread of the debug library instead (test infrastructure: bit-identical to the reference).  Device scores
differ from the reference's only through ``log`` (device math library against the host's).  There is no CPU fallback: without a device
the native library raises.
"""

from __future__ import annotations

import ctypes as C
import logging
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native
from .polyphase import TriangleSparseMatrix

_KIND_SN, _KIND_S2, _KIND_DN = 0, 1, 2

logger = logging.getLogger(__name__)


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
        _native.checked(L, st)
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


def _read_scores(L, h, n: int, stats: Optional[list]) -> List[VariantScoring]:
    """The results of a whamd_progeny_scores handle."""
    out = []
    for k in range(n):
        cnt = L.whamd_progeny_score_count(h, k)
        i = np.empty(cnt, dtype=np.uint32)
        j = np.empty(cnt, dtype=np.uint32)
        s32 = np.empty(cnt, dtype=np.float32)
        s64 = np.empty(cnt, dtype=np.float64)
        if cnt:
            _native.checked(L, L.whamd_progeny_score_get(h, k, _native._ptr(i, C.c_uint32), _native._ptr(j, C.c_uint32), _native._ptr(s32, C.c_float),
                                                         _native._ptr(s64, C.c_double)))
        out.append(VariantScoring(i, j, s32, s64))
        if stats is not None:
            stats.append(_native.read_stats(L, "whamd_progeny_score_get_stats", _native.ProgenyScoreStats, h, k))
    return out


def score_variants_batch(problems: Sequence[ProgenyProblem], device: int = 0, host: bool = False, stats: Optional[list] = None) -> List[VariantScoring]:
    """get_variant_scoring for every problem in one native call (one upload, one launch, one download for the whole batch).  ``stats``,
    if given, receives one dict per problem (counts, and the timings of the whole call)."""
    with _native.batch_handle(host, [p.view() for p in problems], "whamd_progeny_score", "whamd_debug_progeny_score_host", "whamd_progeny_score_destroy",
                              device=device) as (L, h):
        return _read_scores(L, h, len(problems), stats)


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
    _native.checked(L, st)
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
    _native.checked(L, st)
    return list(zip(g0.tolist(), g1.tolist())), llh


# ---------------------------------------------------------------------------------------------- genotype likelihoods from allele depths
def _depths(a, name: str) -> np.ndarray:
    a = np.asarray(a)
    if a.ndim != 2:
        raise ValueError(f"{name} must be [n_samples][n_rows]")
    if a.size and (a.min() < 0 or a.max() > 0xFFFFFFFF):
        raise ValueError(f"{name} holds a depth outside 0 .. 2^32 - 1")
    return np.ascontiguousarray(a, dtype=np.uint32)


class DepthProblem:
    """One call's input for the likelihoods: allele depths ``ref_depth`` / ``alt_depth`` [n_samples][n_rows] (a row is one progeny
    position under one choice of ref / alt allele and parental type), ``ploidy``, ``error_rate``, ``node_row`` [n_nodes] (the row of
    every table row; default: one node per row), ``priors`` [k+1][k+1][k+1] with the rows' ``row_alt_count`` / ``row_co_alt_count`` or
    None.  For :func:`score_variants_from_depths` also what :class:`ProgenyProblem` takes: ``node_variant``, ``alt_count``,
    ``co_alt_count``, ``scoring_window``."""

    def __init__(self, ref_depth, alt_depth, ploidy: int, error_rate: float, node_row=None, priors=None, row_alt_count=None, row_co_alt_count=None,
                 node_variant=None, alt_count=None, co_alt_count=None, scoring_window: int = 0):
        self.ref_depth = _depths(ref_depth, "ref_depth")
        self.alt_depth = _depths(alt_depth, "alt_depth")
        if self.ref_depth.shape != self.alt_depth.shape:
            raise ValueError("ref_depth and alt_depth differ in shape (mismatched lengths)")
        self.n_samples, self.n_rows = self.ref_depth.shape
        self.ploidy = int(ploidy)
        if self.ploidy < 0 or self.ploidy > 0xFFFFFFFE:
            raise ValueError(f"ploidy {ploidy} outside 0 .. 2^32 - 2 (the library refuses a ploidy below 2)")
        self.error_rate = float(error_rate)
        self.node_row = np.ascontiguousarray(np.arange(self.n_rows) if node_row is None else node_row, dtype=np.uint32)
        k1 = self.ploidy + 1
        self.priors = None
        self.row_alt_count = self.row_co_alt_count = None
        if priors is not None:
            self.priors = np.ascontiguousarray(priors, dtype=np.float64)
            if self.priors.shape != (k1, k1, k1):
                raise ValueError(f"priors must be [{k1}][{k1}][{k1}] for ploidy {k1 - 1} (mismatched lengths)")
            if row_alt_count is None or row_co_alt_count is None:
                raise ValueError("priors need row_alt_count and row_co_alt_count")
            self.row_alt_count = np.ascontiguousarray(row_alt_count, dtype=np.uint32)
            self.row_co_alt_count = np.ascontiguousarray(row_co_alt_count, dtype=np.uint32)
            if self.row_alt_count.shape != (self.n_rows,) or self.row_co_alt_count.shape != (self.n_rows,):
                raise ValueError("row_alt_count and row_co_alt_count must have one entry per depth row (mismatched lengths)")
        self.node_variant = None if node_variant is None else np.ascontiguousarray(node_variant, dtype=np.uint32)
        self.alt_count = None if alt_count is None else np.ascontiguousarray(alt_count, dtype=np.uint32)
        self.co_alt_count = None if co_alt_count is None else np.ascontiguousarray(co_alt_count, dtype=np.uint32)
        if self.node_variant is not None and self.node_variant.shape != self.node_row.shape:
            raise ValueError("node_variant and node_row differ in length (mismatched lengths)")
        if (self.alt_count is None) != (self.co_alt_count is None) or (self.alt_count is not None and self.alt_count.shape != self.co_alt_count.shape):
            raise ValueError("alt_count and co_alt_count differ in length (mismatched lengths)")
        self.scoring_window = int(scoring_window)
        if self.scoring_window < 0 or self.scoring_window > 0xFFFFFFFF:
            raise ValueError(f"scoring_window {scoring_window} outside 0 .. 2^32 - 1 (0: likelihoods only; scoring needs at least 4)")

    @property
    def n_nodes(self) -> int:
        return int(self.node_row.size)

    @classmethod
    def from_tables(cls, variant_table, progeny_table, offspring: Sequence[str], varinfo, phasing_param) -> "DepthProblem":
        """From the reference's objects, duck-typed, as get_offspring_gl reads them (offspringscoring.py:93-135): phasable variants whose
        position the progeny table lacks are removed from ``varinfo`` (a position of 0 is never found; of progeny records that share a
        position the last counts), every remaining phasable variant makes ``alt_count`` nodes, and depth rows follow the runs of equal
        progeny position.  ``phasing_param``: ``ploidy``, ``allele_error_rate`` and, for scoring, ``scoring_window``."""
        # the index of every position among the progeny records: of records that share a position the last one counts, a position of 0 none
        record_of = {v.position: i for i, v in enumerate(progeny_table.variants) if v.position}
        for variant in varinfo.get_phasable():
            if variant_table.variants[variant].position not in record_of:
                varinfo.remove_phasable(variant)
        nodes = [int(v) for v in varinfo.get_node_positions()]
        pairs = [(v, record_of[variant_table.variants[v].position]) for v in nodes]
        logger.debug("%d marker nodes over %d progeny records", len(nodes), len(record_of))
        ref, alt, node_row, row_alt, row_co = _depth_rows(progeny_table, list(offspring), pairs, varinfo)
        n_variants = max(nodes) + 1 if nodes else 0
        alt_count = np.zeros(n_variants, dtype=np.uint32)
        co_alt_count = np.zeros(n_variants, dtype=np.uint32)
        for v in set(nodes):
            alt_count[v], co_alt_count[v] = varinfo[v].alt_count, varinfo[v].co_alt_count
        return cls(ref, alt, phasing_param.ploidy, phasing_param.allele_error_rate, node_row=node_row,
                   priors=compute_gt_likelihood_priors(phasing_param.ploidy), row_alt_count=row_alt, row_co_alt_count=row_co, node_variant=nodes,
                   alt_count=alt_count, co_alt_count=co_alt_count, scoring_window=getattr(phasing_param, "scoring_window", 0))

    def view(self) -> _native.ProgenyDepthsView:
        u32 = C.c_uint32
        return _native.ProgenyDepthsView(_native._ptr(self.ref_depth, u32), _native._ptr(self.alt_depth, u32), self.n_rows, self.n_samples, self.ploidy,
                                         self.error_rate, _native._ptr(self.row_alt_count, u32), _native._ptr(self.row_co_alt_count, u32), self.n_nodes,
                                         _native._ptr(self.node_row, u32), _native._ptr(self.priors, C.c_double), self.scoring_window,
                                         _native._ptr(self.node_variant, u32), 0 if self.alt_count is None else self.alt_count.size,
                                         _native._ptr(self.alt_count, u32), _native._ptr(self.co_alt_count, u32))


def _depth_views(problems: Sequence[DepthProblem]):
    views = (_native.ProgenyDepthsView * max(len(problems), 1))()
    for k, p in enumerate(problems):
        views[k] = p.view()
    return views


def offspring_gl_batch(problems: Sequence[DepthProblem], device: int = 0, host: bool = False,
                       doubles: Optional[list] = None) -> List[ProgenyGenotypeLikelihoods]:
    """The ProgenyGenotypeLikelihoods table of every problem -- what get_offspring_gl fills -- in one native call (one upload, one launch,
    one download for the whole batch): the array-level entry for many chromosomes or parents per call.  ``host=True``: the debug
    library's one-thread twin of the kernel (the same function, bit-identical).  ``doubles``, if given, receives per problem the float64
    array the table was rounded from."""
    L = _native.debug_lib() if host else _native.lib()
    n = len(problems)
    tables = [np.empty((p.n_nodes, p.n_samples, p.ploidy + 1), dtype=np.float32) for p in problems]
    f64 = [np.empty(t.shape, dtype=np.float64) for t in tables] if doubles is not None else []
    out32 = (C.POINTER(C.c_float) * max(n, 1))(*[_native._ptr(t, C.c_float) for t in tables])
    out64 = (C.POINTER(C.c_double) * max(n, 1))(*[_native._ptr(t, C.c_double) for t in f64]) if f64 else None
    views = _depth_views(problems)
    if host:
        st = L.whamd_debug_progeny_gl_host(views, n, out32, out64)
    else:
        st = L.whamd_progeny_gl(views, n, int(device), out32, out64)
    _native.checked(L, st)
    if doubles is not None:
        doubles.extend(f64)
    return [ProgenyGenotypeLikelihoods.from_array(t) for t in tables]


def score_variants_from_depths(problems: Sequence[DepthProblem], device: int = 0, stats: Optional[list] = None) -> List[VariantScoring]:
    """get_variant_scoring on the tables of :func:`offspring_gl_batch` for every problem, from allele depths to scores in one native call:
    one upload (depths and entry lists), two launches -- the likelihood kernel writes the packed planes the pair kernel reads -- and one
    download.  No likelihood table exists on the host.  The same entries and bits as :func:`score_variants_batch` on the downloaded
    tables.  ``stats`` as there."""
    for p in problems:
        if p.node_variant is None or p.alt_count is None:
            raise ValueError("scoring needs node_variant, alt_count and co_alt_count")
    with _native.batch_handle(False, [p.view() for p in problems], "whamd_progeny_score_depths", None, "whamd_progeny_score_destroy", device=device) as (L, h):
        return _read_scores(L, h, len(problems), stats)


def _depth_rows(progeny_table, samples: Sequence[str], position_pairs, varinfo):
    """The arrays of compute_gt_likelihoods' loop (offspringscoring.py:245-255): one depth row per run of equal progeny position, read
    with the ref / alt allele and the parental type of the run's first node; an allele index beyond a record's depth tuple counts 0."""
    node_row, rows = [], []
    prev_pos = -1
    for parent_pos, progeny_pos in position_pairs:
        if progeny_pos != prev_pos or not rows:
            v = varinfo[parent_pos]
            rows.append((progeny_pos, v.ref, v.alt, v.alt_count, v.co_alt_count))
            prev_pos = progeny_pos
        node_row.append(len(rows) - 1)
    ref = np.zeros((len(samples), len(rows)), dtype=np.uint32)
    alt = np.zeros((len(samples), len(rows)), dtype=np.uint32)
    for s, sample in enumerate(samples):
        depths = progeny_table.allele_depths_of(sample)
        for r, (pos, a_ref, a_alt, _, _) in enumerate(rows):
            d = depths[pos]
            ref[s, r] = d[a_ref] if len(d) > a_ref else 0
            alt[s, r] = d[a_alt] if len(d) > a_alt else 0
    return ref, alt, np.asarray(node_row, dtype=np.uint32), [r[3] for r in rows], [r[4] for r in rows]


def compute_gt_likelihoods(progeny_table, offspring: str, position_pairs, varinfo, param, gt_priors=None, device: int = 0, host: bool = False):
    """compute_gt_likelihoods (offspringscoring.py:232-274), duck-typed on the reference's ``VariantTable`` (``allele_depths_of``) and
    ``VariantInfo``: per position pair the list of ploidy + 1 likelihoods (doubles), or None where the sample has fewer reads than the
    ploidy; a pair whose progeny position equals that of the pair before it repeats that pair's list.  Turning the objects into arrays
    stays in Python; the likelihoods come from the device (``host=True``: the debug library's twin)."""
    ref, alt, node_row, row_alt, row_co = _depth_rows(progeny_table, [offspring], list(position_pairs), varinfo)
    pri = dict(priors=gt_priors, row_alt_count=row_alt, row_co_alt_count=row_co) if gt_priors is not None and len(gt_priors) else {}
    f64: list = []
    offspring_gl_batch([DepthProblem(ref, alt, param.ploidy, param.allele_error_rate, node_row=node_row, **pri)], device=device, host=host, doubles=f64)
    out: list = []
    for node, row in enumerate(node_row.tolist()):
        if node and row == node_row[node - 1]:
            out.append(out[-1])
        else:
            gl = f64[0][node, 0]
            out.append(None if gl[0] < 0.0 else [float(x) for x in gl])
    return out


def get_offspring_gl(variant_table, progeny_table, offspring: Sequence[str], varinfo, phasing_param, device: int = 0,
                     host: bool = False) -> ProgenyGenotypeLikelihoods:
    """get_offspring_gl (offspringscoring.py:86-140), duck-typed on the reference's ``VariantTable`` (``variants[i].position``,
    ``len``, ``allele_depths_of``) and ``VariantInfo``.  As there: phasable variants whose position the progeny table lacks are removed
    from ``varinfo`` (a position of 0 is never found), every remaining phasable variant makes ``alt_count`` nodes, and a node whose
    progeny position equals that of the node before it reuses that node's likelihoods.  Turning the objects into arrays stays in Python;
    all samples' likelihoods then come from one device call (``host=True``: the debug library's twin)."""
    return offspring_gl_batch([DepthProblem.from_tables(variant_table, progeny_table, offspring, varinfo, phasing_param)], device=device, host=host)[0]


def correct_variant_types(variant_table, progeny_table, offspring: Sequence[str], varinfo, phasing_param, device: int = 0, host: bool = False) -> None:
    """correct_variant_types (offspringscoring.py:37-83): the likelihoods of :func:`get_offspring_gl`, the best fitting parental type of
    every variant's first node (:func:`most_likely_variant_types`), then ``varinfo.correct_type`` for each of them, after the loop as
    the reference applies them."""
    priors = compute_gt_likelihood_priors(phasing_param.ploidy)
    off_gl = get_offspring_gl(variant_table, progeny_table, offspring, varinfo, phasing_param, device=device, host=host)
    node_variant = varinfo.get_node_positions()[: off_gl.getNumPositions()]
    first = [n for n, v in enumerate(node_variant) if n == 0 or v != node_variant[n - 1]]
    winners, _ = most_likely_variant_types(priors, off_gl, nodes=first, device=device, host=host)
    for n, gt in zip(first, winners):   # (all types are chosen before the first is changed, as in the reference)
        varinfo.correct_type(node_variant[n], gt[0], gt[1])
