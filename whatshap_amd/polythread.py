"""Polyphase threading inputs on the device: what ``run_threading`` (whatshap/polyphase/threading.py) computes on both sides of its
threader -- ``get_allele_depths`` (lines 274-317), ``select_clusters`` (228-271), ``compute_readlength_snp_distance_ratio`` (78-82) and
``compute_haplotypes`` (112-131).

Per (position, cluster) the native library leaves the depth of every allele, the rank of the first read of the cluster's list that shows
it (the reference's dict insertion order) and the consensus list; per position the clusters the threader may use, gap filling included.
The transposition, the depths, the consensus lists and the selection run on the device; the sequential gap filling runs on the host
inside the native call.  ``host=True`` takes the one-thread twin of the debug library instead (test infrastructure, the same bytes).
The threader itself, ``HaploThreader.computePaths`` as ``compute_threading_path`` calls it (lines 85-109), is here too:
:func:`thread_batch` runs the DP over the tuples of every column on the device, one workgroup per section, any number of problems in one
call; :func:`compute_threading_path` has the reference's signature and :func:`run_threading` chains inputs, threader and haplotypes
without leaving arrays.  The optimum is the reference's bit for bit; the path is the reference's wherever ``ambiguous`` is 0, and an
optimal one where the reference's own choice hangs on the iteration order of a hash map.  ``force_genotypes`` is not
here: it stays the reference's function (it needs scipy), handed to :func:`run_threading` by the caller.  There is no CPU fallback:
without a device the native call raises.
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


# ---------------------------------------------------------------------------------------------- the threader
class ThreaderProblem:
    """One problem of :func:`thread_batch` at array level: ``cov_ptr`` / ``cov_cluster`` (cov_map as CSR, any order within a position),
    ``pc_ptr`` / ``pc_cluster`` / ``pc_total`` (per (position, cluster) row the depth over all alleles; every listed cluster needs a row),
    ``ploidy`` (2 .. 6), the costs, ``max_cluster_gap``, ``block_starts`` and ``row_limit`` (0)."""

    def __init__(self, cov_ptr, cov_cluster, pc_ptr, pc_cluster, pc_total, ploidy: int, switch_cost: float = 32.0, affine_switch_cost: float = 8.0,
                 max_cluster_gap: int = 10, block_starts=(0,), row_limit: int = 0, want_costs: bool = False):
        self.cov_ptr = np.ascontiguousarray(cov_ptr, dtype=np.uint64)
        self.cov_cluster = np.ascontiguousarray(cov_cluster, dtype=np.uint32)
        self.pc_ptr = np.ascontiguousarray(pc_ptr, dtype=np.uint64)
        self.pc_cluster = np.ascontiguousarray(pc_cluster, dtype=np.uint32)
        self.pc_total = np.ascontiguousarray(pc_total, dtype=np.uint32)
        if len(self.cov_ptr) != len(self.pc_ptr) or len(self.cov_ptr) < 1:
            raise ValueError("cov_ptr and pc_ptr must both hold positions + 1 offsets")
        if len(self.cov_cluster) != int(self.cov_ptr[-1]) or len(self.pc_cluster) != int(self.pc_ptr[-1]) or len(self.pc_total) != len(self.pc_cluster):
            raise ValueError("an array is not as long as its offsets say")
        self.ploidy = int(ploidy)
        if not 0 <= self.ploidy < 1 << 32:
            raise ValueError(f"ploidy {ploidy} outside {_native.POLY_THREADER_MIN_PLOIDY} .. {_native.POLY_THREADER_MAX_PLOIDY}")
        self.switch_cost, self.affine_switch_cost = float(switch_cost), float(affine_switch_cost)
        if max_cluster_gap < 0:
            raise ValueError("max_cluster_gap is negative")
        self.max_cluster_gap = min(int(max_cluster_gap), 0xFFFFFFFF)
        self.block_starts = np.ascontiguousarray(block_starts, dtype=np.uint64)
        if not 0 <= int(row_limit) < 1 << 32:
            raise ValueError(f"row_limit {row_limit}: only 0 (no limit) is supported")
        self.row_limit = int(row_limit)
        self.want_costs = bool(want_costs)

    @classmethod
    def from_inputs(cls, inputs: ThreadingInputs, switch_cost=None, affine_switch_cost=None, max_cluster_gap: int = 10, block_starts=(0,), **kw):
        """From :class:`ThreadingInputs` directly.  A re-added cluster without a row at its position gets one of depth 0 (the reference
        appends an empty dict there); the costs default to those of run_threading."""
        n_pos = len(inputs.pc_ptr) - 1
        total = inputs.pc_depth.sum(axis=1, dtype=np.uint64) if inputs.pc_depth.size else np.zeros(len(inputs.pc_cluster), dtype=np.uint64)
        if total.size and total.max() > 0xFFFFFFFF:
            raise ValueError("a depth outside uint32 (out of range)")
        pc_ptr, pc_cluster, pc_total = inputs.pc_ptr, inputs.pc_cluster, total
        readded = np.flatnonzero(inputs.cov_readded)
        if readded.size:
            pos_of = np.searchsorted(inputs.cov_ptr, readded, side="right") - 1
            row_pos = np.repeat(np.arange(n_pos), np.diff(inputs.pc_ptr).astype(np.int64))
            have = set(zip(row_pos.tolist(), inputs.pc_cluster.tolist()))
            extra = [(int(x), int(inputs.cov_cluster[k])) for x, k in zip(pos_of.tolist(), readded.tolist()) if (int(x), int(inputs.cov_cluster[k])) not in have]
            if extra:
                all_pos = np.concatenate([row_pos, np.asarray([e[0] for e in extra], dtype=np.int64)])
                order = np.argsort(all_pos, kind="stable")
                pc_cluster = np.concatenate([inputs.pc_cluster, np.asarray([e[1] for e in extra], dtype=np.uint32)])[order]
                pc_total = np.concatenate([total, np.zeros(len(extra), dtype=np.uint64)])[order]
                pc_ptr = np.zeros(n_pos + 1, dtype=np.uint64)
                np.cumsum(np.bincount(all_pos, minlength=n_pos), out=pc_ptr[1:])
        return cls(inputs.cov_ptr, inputs.cov_cluster, pc_ptr, pc_cluster, pc_total, inputs.ploidy,
                   inputs.switch_cost if switch_cost is None else switch_cost, inputs.affine_switch_cost if affine_switch_cost is None else affine_switch_cost,
                   max_cluster_gap, block_starts, **kw)

    def view(self) -> _native.PolyThreaderView:
        P = _native._ptr
        return _native.PolyThreaderView(len(self.cov_ptr) - 1, P(self.cov_ptr, C.c_uint64), P(self.cov_cluster, C.c_uint32), P(self.pc_ptr, C.c_uint64),
                                        P(self.pc_cluster, C.c_uint32), P(self.pc_total, C.c_uint32), len(self.block_starts), P(self.block_starts, C.c_uint64),
                                        self.switch_cost, self.affine_switch_cost, self.ploidy, self.max_cluster_gap, self.row_limit,
                                        _native.POLY_THREADER_WANT_COSTS if self.want_costs else 0)


class ThreadingResult:
    """One problem of :func:`thread_batch`: ``paths`` uint32 [n_pos][ploidy] (cluster ids in slot order), per section ``section_first``,
    ``score`` (float32: the optimum, the reference's bit for bit) and ``ambiguous`` (0: the path is the reference's); ``path_cost``
    float32 [n_pos] (the coverage cost of the path's tuple), ``smoothed`` (computeCoverage, per cov_map entry), ``all_costs``
    (``want_costs``: of every tuple, in enumeration order); ``stats``."""

    ARRAYS = ("paths", "path_cost", "smoothed", "section_first", "score", "ambiguous", "all_costs")

    def __init__(self, arrays, stats):
        self.paths, self.path_cost, self.smoothed, self.section_first, self.score, self.ambiguous, self.all_costs = arrays
        self.stats = stats

    def tobytes(self) -> bytes:
        return b"".join(getattr(self, name).tobytes() for name in self.ARRAYS)


def thread_batch(problems: Sequence[ThreaderProblem], device: int = 0, host: bool = False) -> List[ThreadingResult]:
    """Every problem in one native call: one upload, ``_native.POLY_THREADER_LAUNCHES`` launches whatever the problems; the sections of
    all problems are the jobs.  ``IndexError`` for a cov_map cluster without a depth row, as the reference's ``.at()`` gives."""
    P = _native._ptr
    try:
        handle = _native.batch_handle(host, [p.view() for p in problems], "whamd_poly_threader", "whamd_debug_poly_threader_host", "whamd_poly_threader_destroy",
                                      device=device)
        with handle as (L, h):
            out = []
            for k, p in enumerate(problems):
                n_pos, n_sec = L.whamd_poly_threader_position_count(h, k), L.whamd_poly_threader_section_count(h, k)
                n_cov, n_costs = L.whamd_poly_threader_cov_count(h, k), L.whamd_poly_threader_cost_count(h, k)
                arrays = (np.zeros((n_pos, p.ploidy), dtype=np.uint32), np.zeros(n_pos, dtype=np.float32), np.zeros(n_cov, dtype=np.uint32),
                          np.zeros(n_sec, dtype=np.uint64), np.zeros(n_sec, dtype=np.float32), np.zeros(n_sec, dtype=np.uint32), np.zeros(n_costs, dtype=np.float32))
                _native.checked(L, L.whamd_poly_threader_get(h, k, P(arrays[0], C.c_uint32), P(arrays[1], C.c_float), P(arrays[2], C.c_uint32),
                                                             P(arrays[3], C.c_uint64), P(arrays[4], C.c_float), P(arrays[5], C.c_uint32), P(arrays[6], C.c_float)))
                out.append(ThreadingResult(arrays, _native.read_stats(L, "whamd_poly_threader_get_stats", _native.PolyThreaderStats, h, k)))
            return out
    except ValueError as e:
        if "has no depth row" in str(e):
            raise IndexError(str(e)) from e
        raise


def _threader_problem_from_dicts(cov_map, allele_depths, ploidy, switch_cost, affine_switch_cost, max_cluster_gap, **kw) -> ThreaderProblem:
    n_pos = len(cov_map)
    if len(allele_depths) != n_pos:
        raise ValueError("cov_map and allele_depths differ in length")
    cov_ptr, pc_ptr = np.zeros(n_pos + 1, dtype=np.uint64), np.zeros(n_pos + 1, dtype=np.uint64)
    cov, cluster, total = [], [], []
    for x in range(n_pos):
        cov.extend(cov_map[x])
        cov_ptr[x + 1] = len(cov)
        for cid, depths in allele_depths[x].items():
            cluster.append(cid)
            total.append(sum(depths.values()))
        pc_ptr[x + 1] = len(cluster)
    for name, values in (("cluster id", cov), ("cluster id", cluster), ("depth", total)):
        if values and (min(values) < 0 or max(values) > 0xFFFFFFFF):
            raise ValueError(f"a {name} outside uint32 (out of range)")
    return ThreaderProblem(cov_ptr, cov, pc_ptr, cluster, total, ploidy, switch_cost, affine_switch_cost, max_cluster_gap, **kw)


def compute_threading_path(cov_map: List[List[int]], allele_depths: List[Dict[int, Dict[int, int]]], ploidy: int, switch_cost: float = 32.0,
                           affine_switch_cost: float = 8.0, max_cluster_gap: int = 10, *, device: int = 0, host: bool = False) -> List[List[int]]:
    """compute_threading_path (threading.py:85-109): the threading of ``ploidy`` haplotypes through the clusters, one list of cluster
    ids per position.  ``ValueError`` for what the reference would run with a row limit (ploidy above 6) and for switch costs whose
    ``cost(k)`` is not exact in float."""
    if not len(cov_map):
        return []
    problem = _threader_problem_from_dicts(cov_map, allele_depths, ploidy, switch_cost, affine_switch_cost, max_cluster_gap)
    return thread_batch([problem], device=device, host=host)[0].paths.tolist()


def run_threading(allele_matrix: AlleleMatrix, clustering, ploidy: int, genotypes, distrust_genotypes: bool = False, max_cluster_gap: int = 10,
                  error_rate: float = 0.05, *, force_genotypes=None, device: int = 0, host: bool = False):
    """run_threading (threading.py:24-75): ``(paths, haplotypes)``, lists as there.  Inputs, threader and haplotypes stay arrays in
    between.  ``force_genotypes`` is the reference's function (``whatshap.polyphase.threading.force_genotypes``), called as there unless
    ``distrust_genotypes``; without it and with ``distrust_genotypes=False`` this raises instead of skipping the step."""
    if not distrust_genotypes and force_genotypes is None:
        raise ValueError("distrust_genotypes is False: pass force_genotypes (the reference's function); the step is never skipped silently")
    try:
        inputs = threading_inputs_batch([ThreadingProblem(allele_matrix, clustering, ploidy, max_cluster_gap)], device=device, host=host)[0]
    except ValueError as e:
        if "has no counted entry" in str(e):
            raise IndexError("list index out of range") from e
        raise
    n_pos = len(inputs.pc_ptr) - 1
    if not n_pos:
        return [], [[] for _ in range(int(ploidy))]
    result = thread_batch([ThreaderProblem.from_inputs(inputs, max_cluster_gap=max_cluster_gap)], device=device, host=host)[0]
    assert len(result.paths) == n_pos
    paths = result.paths.tolist()
    haplotypes = haplotypes_from_inputs(result.paths, inputs, device=device, host=host).tolist()
    if not distrust_genotypes:
        haplotypes = force_genotypes(paths, haplotypes, genotypes, inputs.cov_map(), inputs.allele_depths(), error_rate)
    return paths, haplotypes
