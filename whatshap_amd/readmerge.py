"""Read merging on the device: ``ReadMerger.merge`` of whatshap/merge.py, the step ``whatshap phase --merge-reads`` runs in front of the
read selection (cli/phase.py:517-534).

Every read is compared with the earlier reads whose window is still open; a pair whose overlap agrees well enough is a blue edge; the
connected components of the blue graph become superreads (per position the summed qualities of both alleles).  The native library
packs the alleles 64 per word on the host, compares all pairs and adds the superreads' sums on the device, and forms the components
(union-find) between the two on the host; ``host=True`` does everything in plain loops on one host thread of the debug library (test
infrastructure).  Every quantity is an integer except one correctly rounded double quotient, so the results equal the reference's.
There is no CPU fallback: without a device the native call raises.

The thresholds are computed here with the reference's own expression and handed down as integers.  When a call reports not-blue edges
(possible only with thresholds below 1) the reference cuts components apart through networkx; :meth:`ReadMerger.merge` does the same
from the device's edge list and calls again with the representatives given.
"""

from __future__ import annotations

import ctypes as C
from math import log
from typing import List, Optional, Sequence

import numpy as np

from . import _native
from .core import Read, ReadSet

LAUNCHES = _native.READMERGE_LAUNCHES
_THRESHOLD_CLAMP = 1 << 40   # every quantity a threshold is compared with lies within +-2^32: clamping to +-2^40 changes no comparison


def thresholds(error_rate: float, positive_threshold, negative_threshold):
    """(thr_diff, thr_neg_diff) as merge.py:78-79 computes them (the same exceptions for the same arguments)."""
    thr_diff = 1 + int(log(positive_threshold, (1 - error_rate) / (error_rate / 3)))
    thr_neg_diff = 1 + int(log(negative_threshold, (1 - error_rate) / (error_rate / 3)))
    return thr_diff, thr_neg_diff


def _clamped(value: int) -> int:
    return max(-_THRESHOLD_CLAMP, min(_THRESHOLD_CLAMP, int(value)))


class MergeProblem:
    """One read set as arrays: the reads, in the order given, as a CSR of (position, allele, quality); the two integer thresholds and
    ``max_error_rate``; optionally ``representative`` (per read the smallest id of its component), which skips pairs and components."""

    def __init__(self, read_ptr, entry_position, entry_allele, entry_quality, thr_diff: int, thr_neg_diff: int, max_error_rate: float, representative=None):
        self.read_ptr = np.ascontiguousarray(read_ptr, dtype=np.uint64)
        if self.read_ptr.size == 0:
            self.read_ptr = np.zeros(1, dtype=np.uint64)
        self.n_reads = self.read_ptr.size - 1
        try:
            self.entry_position = np.ascontiguousarray(np.asarray(entry_position, dtype=np.int64))
            self.entry_quality = np.ascontiguousarray(np.asarray(entry_quality, dtype=np.int64))
        except OverflowError as exc:
            raise _native.SolverError(_native.WHAMD_ERR_UNSUPPORTED, f"a position or a quality beyond int64 ({exc})") from None
        alleles = np.asarray(entry_allele, dtype=np.int64)
        self.entry_allele = np.ascontiguousarray(np.where((alleles == 0) | (alleles == 1), alleles, 255), dtype=np.uint8)
        n_entries = int(self.read_ptr[-1])
        if not (self.entry_position.size == self.entry_allele.size == self.entry_quality.size == n_entries):
            raise ValueError("entry arrays and read_ptr disagree (mismatched lengths)")
        self.thr_diff, self.thr_neg_diff = _clamped(thr_diff), _clamped(thr_neg_diff)
        self.max_error_rate = float(max_error_rate)
        self.representative = None
        if representative is not None:
            rep = np.asarray(representative, dtype=np.int64)
            if rep.size != self.n_reads:
                raise ValueError("representative and read_ptr disagree (mismatched lengths)")
            if rep.size and (rep.min() < 0 or rep.max() >= 1 << 32):
                raise ValueError("a representative outside uint32")
            self.representative = np.ascontiguousarray(rep, dtype=np.uint32)

    @classmethod
    def from_readset(cls, readset, thr_diff: int, thr_neg_diff: int, max_error_rate: float, representative=None) -> "MergeProblem":
        """From duck-typed reads (iteration over variants with ``position``, ``allele``, ``quality``).  Raises what the reference raises,
        at the read where it would: ``AssertionError`` for an allele outside (0, 1), ``IndexError`` for a read without variants."""
        read_ptr, positions, alleles, qualities = [0], [], [], []
        for read in readset:
            n_before = len(positions)
            for variant in read:
                assert variant.allele in (0, 1)
                positions.append(variant.position)
                alleles.append(variant.allele)
                qualities.append(variant.quality)
            if len(positions) == n_before:
                raise IndexError("a read without variants has no first position")
            read_ptr.append(len(positions))
        return cls(read_ptr, positions, alleles, qualities, thr_diff, thr_neg_diff, max_error_rate, representative)

    def with_representative(self, representative) -> "MergeProblem":
        return MergeProblem(self.read_ptr, self.entry_position, self.entry_allele, self.entry_quality, self.thr_diff, self.thr_neg_diff, self.max_error_rate,
                            representative)

    def view(self, want_edges: bool) -> _native.ReadmergeView:
        P = _native._ptr
        return _native.ReadmergeView(self.n_reads, P(self.read_ptr, C.c_uint64), P(self.entry_position, C.c_int64), P(self.entry_allele, C.c_uint8),
                                     P(self.entry_quality, C.c_int64), P(self.representative, C.c_uint32), self.thr_diff, self.thr_neg_diff, self.max_error_rate,
                                     1 if want_edges else 0, 0)


class MergeResult:
    """Per read ``representative`` and ``component_size``; the superreads as a CSR over the reads -- ``super_ptr`` and per entry
    ``position`` (ascending within a superread), ``allele``, ``quality``, ``sum0``, ``sum1``; with ``want_edges`` the blue edges in
    ascending (j, i) as ``edge_j``, ``edge_i``, ``edge_match``, ``edge_mismatch``, ``edge_not_blue``; ``stats``."""

    FIELDS = ("representative", "component_size", "super_ptr", "position", "allele", "quality", "sum0", "sum1")
    EDGE_FIELDS = ("edge_j", "edge_i", "edge_match", "edge_mismatch", "edge_not_blue")

    def __init__(self, fields, edges, stats):
        for name, value in zip(self.FIELDS, fields):
            setattr(self, name, value)
        for name, value in zip(self.EDGE_FIELDS, edges or (None,) * 5):
            setattr(self, name, value)
        self.stats = stats

    def edges(self) -> List[tuple]:
        """[(j, i, match, mismatch, not_blue)] in ascending (j, i)."""
        return list(zip(self.edge_j.tolist(), self.edge_i.tolist(), self.edge_match.tolist(), self.edge_mismatch.tolist(), self.edge_not_blue.tolist()))

    def merged_reads(self, problem: MergeProblem) -> List[tuple]:
        """[(input id, [(position, allele, quality)])] of the output reads: a read alone in its component as it came, a superread at
        its representative, absorbed reads left out."""
        out = []
        ptr, pos, allele, quality = problem.read_ptr.tolist(), problem.entry_position.tolist(), problem.entry_allele.tolist(), problem.entry_quality.tolist()
        sptr, spos, sallele, squality = self.super_ptr.tolist(), self.position.tolist(), self.allele.tolist(), self.quality.tolist()
        for k in range(problem.n_reads):
            if self.component_size[k] == 1:
                out.append((k, list(zip(pos[ptr[k]:ptr[k + 1]], allele[ptr[k]:ptr[k + 1]], quality[ptr[k]:ptr[k + 1]]))))
            elif self.representative[k] == k:
                out.append((k, list(zip(spos[sptr[k]:sptr[k + 1]], sallele[sptr[k]:sptr[k + 1]], squality[sptr[k]:sptr[k + 1]]))))
        return out


def merge_batch(problems: Sequence[MergeProblem], device: int = 0, host: bool = False, want_edges=False, stats: Optional[list] = None) -> List[MergeResult]:
    """Every problem (read set) in one native call: ``LAUNCHES`` launches whatever the problems (4 for the pairs, 5 for the superreads; a
    stage without work launches nothing).  ``want_edges`` is one flag for all problems or one per problem.  ``stats``, if given,
    receives one dict per problem (its counts; launches and times are those of the whole call)."""
    P = _native._ptr
    wants = [bool(want_edges)] * len(problems) if isinstance(want_edges, (bool, int)) else [bool(w) for w in want_edges]
    with _native.batch_handle(host, [p.view(w) for p, w in zip(problems, wants)], "whamd_readmerge", "whamd_debug_readmerge_host", "whamd_readmerge_destroy",
                              device=device) as (L, h):
        out = []
        for k in range(len(problems)):
            n, n_super = L.whamd_readmerge_count(h, k), L.whamd_readmerge_super_count(h, k)
            i64 = lambda: np.zeros(n_super, dtype=np.int64)   # noqa: E731
            fields = (np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32), np.zeros(n + 1, dtype=np.uint64), i64(), np.zeros(n_super, dtype=np.uint8), i64(),
                      i64(), i64())
            _native.checked(L, L.whamd_readmerge_get(h, k, P(fields[0], C.c_uint32), P(fields[1], C.c_uint32), P(fields[2], C.c_uint64), P(fields[3], C.c_int64),
                                                     P(fields[4], C.c_uint8), P(fields[5], C.c_int64), P(fields[6], C.c_int64), P(fields[7], C.c_int64)))
            edges = None
            if wants[k]:
                m = L.whamd_readmerge_edge_count(h, k)
                u32 = lambda: np.zeros(m, dtype=np.uint32)   # noqa: E731
                edges = (u32(), u32(), u32(), u32(), np.zeros(m, dtype=np.uint8))
                _native.checked(L, L.whamd_readmerge_get_edges(h, k, P(edges[0], C.c_uint32), P(edges[1], C.c_uint32), P(edges[2], C.c_uint32), P(edges[3], C.c_uint32),
                                                               P(edges[4], C.c_uint8)))
            rs = _native.read_stats(L, "whamd_readmerge_get_stats", _native.ReadmergeStats, h, k)
            out.append(MergeResult(fields, edges, rs))
            if stats is not None:
                stats.append(dict(rs))
        return out


def cut_components(n_reads: int, edges: Sequence[tuple]) -> np.ndarray:
    """The representatives after the reference's edge removal (merge.py:135-162), from the blue edges [(j, i, match, mismatch,
    not_blue)] in ascending (j, i).  Both graphs are built through networkx in the reference's insertion order -- read i's node, then
    its edges by ascending j -- so its iteration orders, and with them the shortest paths and the edges removed, are the reference's."""
    try:
        import networkx as nx
    except ImportError as exc:
        raise ImportError("the read set has not-blue edges (thresholds below 1): cutting the blue components apart needs networkx, which is not "
                          "installed; the not-blue edges are never ignored") from exc
    by_i = sorted(edges, key=lambda e: (e[1], e[0]))
    blue, not_blue = nx.Graph(), nx.Graph()
    at = 0
    for i in range(n_reads):
        blue.add_node(i)
        not_blue.add_node(i)
        while at < len(by_i) and by_i[at][1] == i:
            j, _, match, mismatch, is_not_blue = by_i[at]
            blue.add_edge(j, i, match=match, mismatch=mismatch)
            if is_not_blue:
                not_blue.add_edge(j, i, match=match, mismatch=mismatch)
            at += 1
    component = {}
    for number, members in enumerate(nx.connected_components(blue)):
        for v in members:
            component[v] = number
    for u, v in not_blue.edges():
        if component[u] != component[v]:
            continue
        while v in nx.node_connected_component(blue, u):
            path = nx.shortest_path(blue, source=u, target=v)
            w, x = min(zip(path[:-1], path[1:]), key=lambda p: blue[p[0]][p[1]]["match"] - blue[p[0]][p[1]]["mismatch"])
            blue.remove_edge(w, x)
    representative = np.arange(n_reads, dtype=np.uint32)
    for members in nx.connected_components(blue):
        representative[list(members)] = min(members)
    return representative


class ReadMergerBase:
    def merge(self, readset):
        raise NotImplementedError


class ReadMerger(ReadMergerBase):
    """``whatshap.merge.ReadMerger``: the same constructor, ``merge(readset)`` returns a ``ReadSet`` of this package's ``Read``s named
    ``read<input id>`` (the ids of absorbed reads are skipped).  ``device`` / ``host`` choose where the call runs; ``stats``, if
    given, receives the dicts of every native call."""

    def __init__(self, error_rate: float, max_error_rate: float, positive_threshold, negative_threshold, *, device: int = 0, host: bool = False,
                 stats: Optional[list] = None):
        self._error_rate = error_rate
        self._max_error_rate = max_error_rate
        self._positive_threshold = positive_threshold
        self._negative_threshold = negative_threshold
        self._device, self._host, self._stats = device, host, stats

    def merged(self, readset):
        """(problem, result) of ``readset``: the arrays behind :meth:`merge`."""
        thr_diff, thr_neg_diff = thresholds(self._error_rate, self._positive_threshold, self._negative_threshold)
        problem = MergeProblem.from_readset(readset, thr_diff, thr_neg_diff, self._max_error_rate)
        might_cut = thr_diff + thr_neg_diff <= 0   # only then can an edge be blue and not blue
        result = merge_batch([problem], device=self._device, host=self._host, want_edges=might_cut, stats=self._stats)[0]
        if result.stats["n_not_blue"]:
            problem = problem.with_representative(cut_components(problem.n_reads, result.edges()))
            result = merge_batch([problem], device=self._device, host=self._host, stats=self._stats)[0]
        return problem, result

    def merge(self, readset) -> ReadSet:
        problem, result = self.merged(readset)
        return to_readset(result.merged_reads(problem))


def to_readset(merged_reads, read_class=Read, readset_class=ReadSet):
    out = readset_class()
    for k, variants in merged_reads:
        read = read_class(f"read{k}")
        for position, allele, quality in variants:
            read.add_variant(position, allele, quality)
        out.add(read)
    return out


class DoNothingReadMerger(ReadMergerBase):
    def merge(self, readset):
        return readset
