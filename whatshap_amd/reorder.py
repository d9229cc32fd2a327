"""Polyphase reordering on the device: ``whatshap.polyphase.reorder`` (whatshap/polyphase/reorder.py) for the third phase of
``whatshap polyphase`` without prephasing -- ``compute_link_likelihoods``, ``get_optimal_assignments``, ``permute_blocks`` and
``compute_breakpoint_confidence`` behind ``run_reordering``.

Windows and read lists are found on the host inside the native library, the left / right table and every permutation's sum on the device,
the choice of permutations, the permuted threads and haplotypes and the confidences on the host again; ``host=True`` runs the device's part
in the debug library on one host thread instead (test infrastructure, bit-identical to the device).  The link likelihoods equal the
reference's bit for bit: the library takes ``math.log(1 - error_rate)`` and ``math.log(error_rate)`` from here and calls no ``log`` itself.
There is no CPU fallback: without a device the native library raises.

The reference walks the reads of ``{threads[pos][h] for h in affected} | {threads[pos - 1][h] for h in affected}`` in the iteration order
of that Python set.  The array-level call (:func:`link_likelihoods_batch`) takes the clusters of every breakpoint as an explicit ordered
list; the reference-signature functions fill it by evaluating the same expression.
"""

from __future__ import annotations

import ctypes as C
import itertools as it
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _native
from .polyphase import AlleleMatrix


class PhaseBreakpoint:
    """whatshap.polyphase.PhaseBreakpoint."""

    def __init__(self, position: int, haplotypes: List[int], confidence: float):
        self.position = position
        self.haplotypes = sorted(haplotypes[:])
        self.confidence = confidence


def _csr(lists, dtype) -> Tuple[np.ndarray, np.ndarray]:
    ptr = np.zeros(len(lists) + 1, dtype=np.uint64)
    if len(lists):
        np.cumsum([len(x) for x in lists], out=ptr[1:])
    flat = np.fromiter((v for x in lists for v in x), dtype=np.int64, count=int(ptr[-1]))
    if flat.size and (flat.min() < 0 or flat.max() > 0xFFFFFFFF):
        raise ValueError("id outside [0, 2^32)")
    return ptr, np.ascontiguousarray(flat, dtype=dtype)


class ReorderProblem:
    """One block for :func:`link_likelihoods_batch`: the arrays behind a ``whamd_poly_reorder_view``.

    ``threads`` is [n_pos][ploidy], ``haplotypes`` [ploidy][n_pos], ``clustering`` a list of lists of read ids; per breakpoint a position,
    the sorted affected haplotypes and the clusters whose reads are walked, in that order."""

    def __init__(self, allele_matrix: AlleleMatrix, threads, haplotypes, clustering, bp_position: Sequence[int], bp_affected: Sequence[Sequence[int]],
                 bp_clusters: Sequence[Sequence[int]]):
        self.allele_matrix = allele_matrix
        self.haplotypes = np.ascontiguousarray(haplotypes, dtype=np.int8)
        if self.haplotypes.ndim != 2:
            self.haplotypes = self.haplotypes.reshape(len(haplotypes), -1)
        self.ploidy, self.n_pos = self.haplotypes.shape
        self.threads = np.ascontiguousarray(threads, dtype=np.int32).reshape(self.n_pos, self.ploidy)
        self.cluster_ptr, self.cluster_reads = _csr(clustering, np.uint32)
        self.bp_position = np.ascontiguousarray(bp_position, dtype=np.int64)
        if self.bp_position.size and self.bp_position.min() < 0:
            raise ValueError("negative breakpoint position")
        self.bp_position = self.bp_position.astype(np.uint64)
        if not (len(bp_position) == len(bp_affected) == len(bp_clusters)):
            raise ValueError("bp_position, bp_affected and bp_clusters differ in length")
        self.bp_affected_ptr, self.bp_affected = _csr(bp_affected, np.uint32)
        self.bp_cluster_ptr, self.bp_clusters = _csr(bp_clusters, np.uint32)

    def view(self) -> _native.PolyReorderView:
        p = _native._ptr
        return _native.PolyReorderView(self.allele_matrix.view(), self.ploidy, 0, self.n_pos, p(self.haplotypes, C.c_int8), p(self.threads, C.c_int32),
                                       len(self.cluster_ptr) - 1, p(self.cluster_ptr, C.c_uint64), p(self.cluster_reads, C.c_uint32),
                                       len(self.bp_position), p(self.bp_position, C.c_uint64), p(self.bp_affected_ptr, C.c_uint64),
                                       p(self.bp_affected, C.c_uint32), p(self.bp_cluster_ptr, C.c_uint64), p(self.bp_clusters, C.c_uint32))


class ReorderResult:
    """What one problem of :func:`link_likelihoods_batch` returns.

    ``llh[b]``: the k! link log likelihoods of breakpoint b in permutation order; ``best[b]``: the rank of the first largest;
    ``windows[b]``: (left positions, right positions); ``assignments``: [n_breakpoints + 1][ploidy]; ``threads`` / ``haplotypes``: after
    permute_blocks; ``confidence[b]``."""

    def __init__(self, llh_ptr, llh, best, window_ptr, left_count, window, assignments, threads, haplotypes, confidence):
        self.llh_ptr, self.llh_flat, self.best = llh_ptr, llh, best
        self.llh = [llh[int(llh_ptr[b]):int(llh_ptr[b + 1])] for b in range(len(best))]
        self.windows = []
        for b in range(len(best)):
            w = window[int(window_ptr[b]):int(window_ptr[b + 1])].tolist()
            self.windows.append((w[:int(left_count[b])], w[int(left_count[b]):]))
        self.assignments, self.threads, self.haplotypes, self.confidence = assignments, threads, haplotypes, confidence


def link_likelihoods_batch(problems: Sequence[ReorderProblem], error_rate: float = 0.07, device: int = 0, host: bool = False,
                           stats: Optional[list] = None) -> List[ReorderResult]:
    """The reordering of every problem in one native call (one upload, at most two launches, one download for the whole batch).
    ``stats``, if given, receives one dict per problem (counts, and the launches and timings of the whole call)."""
    p = _native._ptr
    with _native.batch_handle(host, [pr.view() for pr in problems], "whamd_poly_reorder", "whamd_debug_poly_reorder_host", "whamd_poly_reorder_destroy",
                              math.log(1 - error_rate), math.log(error_rate), device=device) as (L, h):
        out = []
        for k, pr in enumerate(problems):
            n_bp = L.whamd_poly_reorder_breakpoint_count(h, k)
            llh_ptr = np.zeros(n_bp + 1, dtype=np.uint64)
            llh = np.empty(L.whamd_poly_reorder_llh_count(h, k), dtype=np.float64)
            best = np.empty(n_bp, dtype=np.uint32)
            window_ptr = np.zeros(n_bp + 1, dtype=np.uint64)
            left_count = np.empty(n_bp, dtype=np.uint32)
            window = np.empty(L.whamd_poly_reorder_window_count(h, k), dtype=np.uint32)
            assignments = np.empty((n_bp + 1, pr.ploidy), dtype=np.uint32)
            threads = np.empty((pr.n_pos, pr.ploidy), dtype=np.int32)
            haplotypes = np.empty((pr.ploidy, pr.n_pos), dtype=np.int8)
            confidence = np.empty(n_bp, dtype=np.float64)
            for st in (L.whamd_poly_reorder_get_llh(h, k, p(llh_ptr, C.c_uint64), p(llh, C.c_double), p(best, C.c_uint32)),
                       L.whamd_poly_reorder_get_windows(h, k, p(window_ptr, C.c_uint64), p(left_count, C.c_uint32), p(window, C.c_uint32)),
                       L.whamd_poly_reorder_get_phasing(h, k, p(assignments, C.c_uint32), p(threads, C.c_int32), p(haplotypes, C.c_int8),
                                                        p(confidence, C.c_double))):
                _native.checked(L, st)
            out.append(ReorderResult(llh_ptr, llh, best, window_ptr, left_count, window, assignments, threads, haplotypes, confidence))
            if stats is not None:
                stats.append(_native.read_stats(L, "whamd_poly_reorder_get_stats", _native.PolyReorderStats, h, k))
        return out


# ---------------------------------------------------------------------------------------------- the reference's signatures
def _mirror(allele_matrix) -> AlleleMatrix:
    """Our AlleleMatrix, or one built from the rows of an object with WhatsHap's AlleleMatrix interface."""
    if isinstance(allele_matrix, AlleleMatrix):
        return allele_matrix
    positions = allele_matrix.getPositions()
    read_ptr, pos, alle = [0], [], []
    for r in range(len(allele_matrix)):
        for j, a in allele_matrix.getRead(r):
            pos.append(positions[j])
            alle.append(a)
        read_ptr.append(len(pos))
    return AlleleMatrix.from_csr(read_ptr, pos, alle)


def _problem(threads, haplotypes, breakpoints, clustering, allele_matrix) -> ReorderProblem:
    bp_clusters = []
    for pos, affected in [(b.position, b.haplotypes) for b in breakpoints]:
        affected_clusts = {threads[pos][h] for h in affected}
        if pos > 0:
            affected_clusts = affected_clusts.union({threads[pos - 1][h] for h in affected})
        bp_clusters.append([cid for cid in affected_clusts])   # the set's own iteration order
    return ReorderProblem(_mirror(allele_matrix), threads, haplotypes, clustering, [b.position for b in breakpoints],
                          [list(b.haplotypes) for b in breakpoints], bp_clusters)


def compute_link_likelihoods(threads, haplotypes, breakpoints, clustering, allele_matrix, error_rate, device: int = 0,
                             host: bool = False) -> List[Dict[Tuple[int, ...], float]]:
    """reorder.compute_link_likelihoods (reorder.py:220-292): per breakpoint a dict from each permutation of the affected haplotypes, in
    ``itertools.permutations`` order, to its link log likelihood."""
    if not breakpoints:
        return []
    res = link_likelihoods_batch([_problem(threads, haplotypes, breakpoints, clustering, allele_matrix)], error_rate, device=device, host=host)[0]
    return [dict(zip(it.permutations(b.haplotypes), res.llh[k].tolist())) for k, b in enumerate(breakpoints)]


def get_heterozygous_pos_for_haps(haplotypes, subset, pivot_pos: int, limit: int = 0) -> Tuple[List[int], List[int]]:
    """reorder.get_heterozygous_pos_for_haps (reorder.py:351-376): up to ``limit`` positions below the pivot and up to ``limit`` from it on
    at which the haplotypes of ``subset`` carry at least two values.  (Host arithmetic; the native call finds its windows itself.)"""
    sub = np.asarray([haplotypes[h] for h in subset])
    het = np.flatnonzero((sub != sub[0]).any(axis=0)) if len(subset) else np.zeros(0, dtype=np.int64)
    cut = int(np.searchsorted(het, pivot_pos))
    limit = max(int(limit), 0)
    return het[max(cut - limit, 0):cut].tolist(), het[cut:cut + limit].tolist()


def find_breakpoints(threads) -> List[PhaseBreakpoint]:
    """reorder.find_breakpoints (reorder.py:197-217): positions p at which at least two haplotypes sit, at p - 1, on clusters that some
    haplotype leaves between p - 1 and p."""
    t = np.asarray(threads)
    if t.ndim != 2 or len(t) < 2:
        return []
    out = []
    changed = t[1:] != t[:-1]
    for i in (np.flatnonzero(changed.any(axis=1)) + 1).tolist():
        left = t[i - 1]
        affected = np.flatnonzero(np.isin(left, left[changed[i - 1]])).tolist()
        if len(affected) >= 2:
            out.append(PhaseBreakpoint(i, affected, 0.0))
    return out


def get_optimal_assignments(breakpoints, lllh, ploidy: int, affiliations=None) -> List[List[int]]:
    """reorder.get_optimal_assignments without affiliations (reorder.py:389-407): per breakpoint the first most likely permutation,
    chained from the identity."""
    if affiliations:
        raise NotImplementedError("the ILP over prephasing affiliations is not part of this library; feed compute_link_likelihoods' result to the reference's")
    if not breakpoints:
        return [list(range(ploidy))]
    assignments = [list(range(ploidy)) for _ in range(len(breakpoints) + 1)]
    for b in range(len(breakpoints)):
        assignments[b + 1] = list(assignments[b])
        perm = max(lllh[b], key=lllh[b].get)
        for left, right in zip(sorted(perm), perm):
            assignments[b + 1][assignments[b].index(left)] = right
    return assignments


def run_reordering(allele_matrix, clustering, threads, haplotypes, breakpoints, prephasing, error_rate=0.07, device: int = 0, host: bool = False):
    """reorder.run_reordering (reorder.py:139-194) without prephasing: ``threads`` and ``haplotypes`` are permuted in place, block by
    block, every breakpoint's ``confidence`` is set."""
    if prephasing:
        raise NotImplementedError("reordering with a prephasing solves an ILP that is not part of this library: compute_link_likelihoods "
                                  "returns what the reference's get_optimal_assignments reads")
    res = link_likelihoods_batch([_problem(threads, haplotypes, breakpoints, clustering, allele_matrix)], error_rate, device=device, host=host)[0]
    new_threads, new_haps = res.threads.tolist(), res.haplotypes.tolist()
    for p in range(len(threads)):
        threads[p] = new_threads[p]
    for t in range(len(haplotypes)):
        for p in range(len(new_haps[t])):
            haplotypes[t][p] = new_haps[t][p]
    for bp, conf in zip(breakpoints, res.confidence.tolist()):
        bp.confidence = conf
