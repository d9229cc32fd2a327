"""Polyphase threading inputs on the device: what ``run_threading`` (whatshap/polyphase/threading.py) computes on both sides of its
threader -- ``get_allele_depths`` (lines 274-317), ``select_clusters`` (228-271), ``compute_readlength_snp_distance_ratio`` (78-82) and
``compute_haplotypes`` (112-131).

Per (position, cluster) the native library leaves the depth of every allele, the rank of the first read of the cluster's list that shows
it (the reference's dict insertion order) and the consensus list; per position the clusters the threader may use, gap filling included.
The transposition, the depths, the consensus lists and the selection run on the device; the sequential gap filling runs on the host
inside the native call.  ``host=True`` takes the one-thread twin of the debug library instead (test infrastructure, the same bytes).
``HaploThreader`` and ``force_genotypes`` are not here: a caller runs the reference's threader between :func:`select_clusters` and
:func:`compute_haplotypes`, on what :func:`threading_inputs` returns.  There is no CPU fallback: without a device the native call raises.
"""

from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _native
from .polyphase import AlleleMatrix

NO_READ = np.uint32(0xFFFFFFFF)   # ``pc_first`` of an allele no read of the cluster shows


class ThreadingProblem:
    """One block: the allele matrix, the clustering (a list of lists of read ids, every list in its own order), the ploidy and
    ``max_cluster_gap``.  ``n_alleles`` defaults to the matrix's largest allele + 1."""

    def __init__(self, allele_matrix: AlleleMatrix, clustering: Sequence[Sequence[int]], ploidy: int, max_cluster_gap: int = 10, n_alleles: Optional[int] = None,
                 depths_only: bool = False):
        self.matrix = allele_matrix
        sizes = np.fromiter((len(c) for c in clustering), dtype=np.uint64, count=len(clustering))
        self.cluster_ptr = np.zeros(len(clustering) + 1, dtype=np.uint64)
        np.cumsum(sizes, out=self.cluster_ptr[1:])
        reads = np.concatenate([np.asarray(c, dtype=np.int64).reshape(-1) for c in clustering]) if len(clustering) else np.zeros(0, dtype=np.int64)
        if reads.size and (reads.min() < 0 or reads.max() >= 1 << 32):
            raise ValueError("a read id outside uint32 (out of range)")
        self.cluster_reads = np.ascontiguousarray(reads, dtype=np.uint32)
        self.ploidy = int(ploidy)
        if not 0 <= self.ploidy < 1 << 32:
            raise ValueError(f"ploidy {ploidy} outside 1 .. {_native.POLY_THREAD_MAX_PLOIDY}")
        if max_cluster_gap < 0:
            raise ValueError("max_cluster_gap is negative")
        self.max_cluster_gap = min(int(max_cluster_gap), 0xFFFFFFFF)
        if n_alleles is None:
            n_alleles = max(int(allele_matrix.allele.max()) + 1 if allele_matrix.allele.size else 1, 1)
        self.n_alleles = int(n_alleles)
        self.depths_only = bool(depths_only)

    def view(self) -> _native.PolyThreadView:
        P = _native._ptr
        return _native.PolyThreadView(self.matrix.view(), len(self.cluster_ptr) - 1, P(self.cluster_ptr, C.c_uint64), P(self.cluster_reads, C.c_uint32),
                                      self.ploidy, self.max_cluster_gap, self.n_alleles, _native.POLY_THREAD_DEPTHS_ONLY if self.depths_only else 0)


class ThreadingInputs:
    """The arrays of one problem.  Rows, one per (position, cluster) with a read of the cluster at the position: ``pc_ptr`` [n_pos + 1],
    ``pc_cluster`` (ascending within a position), ``pc_depth`` [rows][n_alleles] (after the gap filling emptied what it empties),
    ``pc_first`` [rows][n_alleles] (rank in the cluster's list of the first read with the allele, ``NO_READ``: none), ``pc_consensus``
    [rows][ploidy].  Lists: ``cov_ptr`` [n_pos + 1], ``cov_cluster`` (ascending), ``cov_readded``, ``cov_rank`` (place before the final
    sort).  ``switch_cost``, ``affine_switch_cost``; ``stats``."""

    def __init__(self, ploidy, n_alleles, rows, cov, costs, stats):
        self.ploidy, self.n_alleles = ploidy, n_alleles
        self.pc_ptr, self.pc_cluster, self.pc_depth, self.pc_first, self.pc_consensus = rows
        self.cov_ptr, self.cov_cluster, self.cov_readded, self.cov_rank = cov
        self.affine_switch_cost, self.switch_cost = costs
        self.stats = stats

    ARRAYS = ("pc_ptr", "pc_cluster", "pc_depth", "pc_first", "pc_consensus", "cov_ptr", "cov_cluster", "cov_readded", "cov_rank")

    def tobytes(self) -> bytes:
        return b"".join(getattr(self, name).tobytes() for name in self.ARRAYS)

    # ---- the reference's forms
    def allele_depths(self) -> List[Dict[int, Dict[int, int]]]:
        """``allele_depths`` as select_clusters leaves it: inner dicts in the reference's insertion order, an emptied row as ``{}``, a
        re-added cluster without a row as ``{}`` behind the position's rows, in the order of appending."""
        return self._dicts()[0]

    def consensus_lists(self) -> List[Dict[int, List[int]]]:
        return self._dicts()[1]

    def cov_map(self) -> List[List[int]]:
        ptr = self.cov_ptr.tolist()
        flat = self.cov_cluster.tolist()
        return [flat[ptr[x]:ptr[x + 1]] for x in range(len(ptr) - 1)]

    def _dicts(self):
        n_pos = len(self.pc_ptr) - 1
        ptr = self.pc_ptr.tolist()
        cluster = self.pc_cluster.tolist()
        order = np.argsort(self.pc_first, axis=1, kind="stable").tolist() if len(cluster) else []
        depth, first, cons = self.pc_depth.tolist(), self.pc_first.tolist(), self.pc_consensus.tolist()
        none = int(NO_READ)
        ad, cl = [], []
        for x in range(n_pos):
            d, c = {}, {}
            for row in range(ptr[x], ptr[x + 1]):
                d[cluster[row]] = {a: depth[row][a] for a in order[row] if first[row][a] != none and depth[row][a]}
                c[cluster[row]] = cons[row]
            ad.append(d)
            cl.append(c)
        cptr, ccl, cre, crk = self.cov_ptr.tolist(), self.cov_cluster.tolist(), self.cov_readded.tolist(), self.cov_rank.tolist()
        for x in range(len(cptr) - 1):
            for _, cid in sorted((crk[k], ccl[k]) for k in range(cptr[x], cptr[x + 1]) if cre[k]):
                ad[x][cid] = {}   # (replaced in place where the cluster had a row, else appended)
        return ad, cl


def compute_readlength_snp_distance_ratio(allele_matrix) -> float:
    """compute_readlength_snp_distance_ratio (threading.py:78-82); ``ZeroDivisionError`` for a matrix without reads, as there."""
    length = 0
    for read in allele_matrix:
        length += len(read)
    return length / len(allele_matrix)


def _switch_costs(n_entries: int, n_reads: int) -> Tuple[int, int]:
    """(affine_switch_cost, switch_cost) of run_threading (threading.py:55-60): ``n_entries`` row entries, what ``len(read)`` sums to,
    over ``n_reads`` reads, with the reference's expression."""
    from math import ceil

    if not n_reads:
        return 0, 0
    affine = ceil(n_entries / n_reads / 1.0)
    return affine, 4 * affine


def threading_inputs_batch(problems: Sequence[ThreadingProblem], device: int = 0, host: bool = False, stats: Optional[list] = None) -> List[ThreadingInputs]:
    """Every problem (block) in one native call: one upload, ``_native.POLY_THREAD_LAUNCHES`` launches whatever the problems.  ``stats``,
    if given, receives one dict per problem (its counts; launches and times are those of the whole call)."""
    P = _native._ptr
    with _native.batch_handle(host, [p.view() for p in problems], "whamd_poly_thread_inputs", "whamd_debug_poly_thread_inputs_host",
                              "whamd_poly_thread_destroy", device=device) as (L, h):
        out = []
        for k, p in enumerate(problems):
            n_pos, n_rows, n_cov = L.whamd_poly_thread_position_count(h, k), L.whamd_poly_thread_row_count(h, k), L.whamd_poly_thread_cov_count(h, k)
            rows = (np.zeros(n_pos + 1, dtype=np.uint64), np.zeros(n_rows, dtype=np.uint32), np.zeros((n_rows, p.n_alleles), dtype=np.uint32),
                    np.zeros((n_rows, p.n_alleles), dtype=np.uint32), np.zeros((n_rows, p.ploidy), dtype=np.int8))
            _native.checked(L, L.whamd_poly_thread_get_rows(h, k, P(rows[0], C.c_uint64), P(rows[1], C.c_uint32), P(rows[2], C.c_uint32), P(rows[3], C.c_uint32),
                                                  P(rows[4], C.c_int8)))
            cov = (np.zeros(n_pos + 1, dtype=np.uint64), np.zeros(n_cov, dtype=np.uint32), np.zeros(n_cov, dtype=np.uint8), np.zeros(n_cov, dtype=np.uint32))
            _native.checked(L, L.whamd_poly_thread_get_cov(h, k, P(cov[0], C.c_uint64), P(cov[1], C.c_uint32), P(cov[2], C.c_uint8), P(cov[3], C.c_uint32)))
            ts = _native.read_stats(L, "whamd_poly_thread_get_stats", _native.PolyThreadStats, h, k)
            out.append(ThreadingInputs(p.ploidy, p.n_alleles, rows, cov, _switch_costs(ts["n_entries"], ts["n_reads"]), ts))
            if stats is not None:
                stats.append(dict(ts))
        return out


# ---------------------------------------------------------------------------------------------- the reference's signatures
def get_allele_depths(allele_matrix: AlleleMatrix, clustering, ploidy: int, *, device: int = 0, host: bool = False):
    """get_allele_depths (threading.py:274-317): ``(ad, cons_lists)``, lists over the positions of dicts over the clusters; a position no
    read of a cluster covers has empty dicts, as there."""
    res = threading_inputs_batch([ThreadingProblem(allele_matrix, clustering, ploidy, 0, depths_only=True)], device=device, host=host)[0]
    return res._dicts()


def select_clusters(allele_depths: List[Dict[int, Dict[int, int]]], ploidy: int, max_gap: int, *, device: int = 0, host: bool = False) -> List[List[int]]:
    """select_clusters (threading.py:228-271): returns ``cov_map`` and empties ``allele_depths[pos][cid]`` of every re-added cluster, as the
    reference does.  ``IndexError`` for a position without a cluster and ``ZeroDivisionError`` for one whose depths are all zero, both
    before anything is changed, as there."""
    n_pos = len(allele_depths)
    ptr = np.zeros(n_pos + 1, dtype=np.uint64)
    cluster, total = [], []
    for x, per_cluster in enumerate(allele_depths):
        if not per_cluster:
            raise IndexError("list index out of range")
        sums = [sum(d.values()) for d in per_cluster.values()]
        if len(sums) > 1 and sum(sums) == 0:
            raise ZeroDivisionError("division by zero")
        cluster.extend(per_cluster.keys())
        total.extend(sums)
        ptr[x + 1] = len(cluster)
    cl = np.asarray(cluster, dtype=np.int64)
    tt = np.asarray(total, dtype=np.int64)
    if cl.size and (cl.min() < 0 or cl.max() >= 0xFFFFFFFF):
        raise ValueError("a cluster id outside uint32 (out of range)")
    if tt.size and (tt.min() < 0 or tt.max() > 0xFFFFFFFF):
        raise ValueError("a depth outside uint32 (out of range)")
    cl, tt = np.ascontiguousarray(cl, dtype=np.uint32), np.ascontiguousarray(tt, dtype=np.uint32)
    if max_gap < 0:
        max_gap = 0   # (range(min(max_gap, ...)) is empty)
    cap = n_pos * (int(ploidy) + 2)
    cov_ptr, cov_cluster, cov_readded, cov_rank = np.zeros(n_pos + 1, dtype=np.uint64), np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint8), np.zeros(cap, dtype=np.uint32)
    L = _native.debug_lib() if host else _native.lib()
    P = _native._ptr
    args = (n_pos, P(ptr, C.c_uint64), P(cl, C.c_uint32), P(tt, C.c_uint32), int(ploidy), min(int(max_gap), 0xFFFFFFFF))
    outs = (P(cov_ptr, C.c_uint64), P(cov_cluster, C.c_uint32), P(cov_readded, C.c_uint8), P(cov_rank, C.c_uint32))
    if host:
        st = L.whamd_debug_poly_select_clusters_host(*args, *outs)
    else:
        launches = C.c_uint32()
        st = L.whamd_poly_select_clusters(*args, int(device), *outs, C.byref(launches))
    _native.checked(L, st)
    cptr, ccl, cre, crk = cov_ptr.tolist(), cov_cluster.tolist(), cov_readded.tolist(), cov_rank.tolist()
    cov_map = []
    for x in range(n_pos):
        cov_map.append(ccl[cptr[x]:cptr[x + 1]])
        for _, cid in sorted((crk[k], ccl[k]) for k in range(cptr[x], cptr[x + 1]) if cre[k]):
            allele_depths[x][cid] = dict()
    return cov_map


def compute_haplotypes(path, consensus_lists: List[Dict[int, List[int]]], ploidy: int, *, device: int = 0, host: bool = False) -> List[List[int]]:
    """compute_haplotypes (threading.py:112-131): ``ploidy`` lists over the positions of the path."""
    n_pos = len(path)
    ploidy = int(ploidy)
    if not n_pos or ploidy < 1:
        return [[] for _ in range(ploidy)]
    paths = np.asarray([list(p[:ploidy]) for p in path], dtype=np.int64).reshape(n_pos, ploidy)
    if paths.min() < 0 or paths.max() >= 0xFFFFFFFF:
        raise ValueError("a cluster id outside uint32 (out of range)")
    paths = np.ascontiguousarray(paths, dtype=np.uint32)
    short = -128   # a pick a list is too short for: IndexError if a slot asks for it, as in the reference
    ptr = np.zeros(n_pos + 1, dtype=np.uint64)
    cluster, cons = [], []
    for x in range(n_pos):
        for cid, picks in consensus_lists[x].items():
            if not 0 <= cid < 0xFFFFFFFF:
                continue   # (no slot can name it)
            picks = list(picks[:ploidy])
            if any(not -127 <= a <= 127 for a in picks):
                raise ValueError("an allele outside int8 (out of range)")
            cluster.append(cid)
            cons.append(picks + [short] * (ploidy - len(picks)))
        ptr[x + 1] = len(cluster)
    cl = np.ascontiguousarray(cluster, dtype=np.uint32)
    cs = np.ascontiguousarray(np.asarray(cons, dtype=np.int8).reshape(len(cluster), ploidy))
    out = np.zeros((ploidy, n_pos), dtype=np.int8)
    L = _native.debug_lib() if host else _native.lib()
    P = _native._ptr
    args = (P(paths, C.c_uint32), n_pos, ploidy, P(ptr, C.c_uint64), P(cl, C.c_uint32), P(cs, C.c_int8))
    if host:
        st = L.whamd_debug_poly_haplotypes_host(*args, P(out, C.c_int8))
    else:
        launches = C.c_uint32()
        st = L.whamd_poly_haplotypes(*args, int(device), P(out, C.c_int8), C.byref(launches))
    _native.checked(L, st)
    if (out == short).any():
        raise IndexError("list index out of range")
    return out.tolist()


def haplotypes_from_inputs(path, inputs: ThreadingInputs, *, device: int = 0, host: bool = False) -> np.ndarray:
    """compute_haplotypes on the arrays of :func:`threading_inputs_batch`, without dicts: int8 [ploidy][n_pos]."""
    n_pos = len(inputs.pc_ptr) - 1
    paths = np.ascontiguousarray(np.asarray(path, dtype=np.int64).reshape(n_pos, inputs.ploidy), dtype=np.uint32)
    out = np.zeros((inputs.ploidy, n_pos), dtype=np.int8)
    L = _native.debug_lib() if host else _native.lib()
    P = _native._ptr
    args = (P(paths, C.c_uint32), n_pos, inputs.ploidy, P(inputs.pc_ptr, C.c_uint64), P(inputs.pc_cluster, C.c_uint32), P(inputs.pc_consensus, C.c_int8))
    if host:
        st = L.whamd_debug_poly_haplotypes_host(*args, P(out, C.c_int8))
    else:
        launches = C.c_uint32()
        st = L.whamd_poly_haplotypes(*args, int(device), P(out, C.c_int8), C.byref(launches))
    _native.checked(L, st)
    return out


def threading_inputs(allele_matrix: AlleleMatrix, clustering, ploidy: int, max_cluster_gap: int = 10, *, device: int = 0, host: bool = False,
                     stats: Optional[list] = None) -> dict:
    """get_allele_depths, select_clusters and the switch costs of run_threading from one fused call, in the shapes
    ``HaploThreader.computePathsBlockwise([0], cov_map, allele_depths)`` takes: ``cov_map``, ``allele_depths`` (as select_clusters leaves
    them), ``cons_lists``, ``switch_cost``, ``affine_switch_cost``.  ``IndexError`` for a position no read of a cluster covers, as
    select_clusters raises there."""
    try:
        res = threading_inputs_batch([ThreadingProblem(allele_matrix, clustering, ploidy, max_cluster_gap)], device=device, host=host, stats=stats)[0]
    except ValueError as e:
        if "has no counted entry" in str(e):
            raise IndexError("list index out of range") from e
        raise
    ad, cl = res._dicts()
    return {"cov_map": res.cov_map(), "allele_depths": ad, "cons_lists": cl, "switch_cost": res.switch_cost, "affine_switch_cost": res.affine_switch_cost}
