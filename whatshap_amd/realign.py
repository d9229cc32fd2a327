"""Allele detection by re-alignment on the device: ``ReadSetReader.detect_alleles_by_alignment`` (whatshap/variants.py:848-912) and the two
distances it uses, ``edit_distance`` and ``edit_distance_affine_gap`` (whatshap/align.pyx:16-196).

The inputs are duck-typed: an alignment needs ``.reference_start``, ``.cigartuples`` and ``.query_sequence``; a variant ``.position``,
``.reference_allele`` and ``.get_alt_allele_list()``; a restriction ``.as_vector()`` or is a plain sequence of allele indices.  The
reference is a ``str`` or ``bytes`` of the whole chromosome.  Results equal the reference's for every input, ties included; its
exceptions are raised with the same types (``ValueError``, ``AssertionError``, ``IndexError``, ``TypeError``).  There is no CPU
fallback: without a device the native library raises.
"""

from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import numpy as np

from . import _native

_EXCEPTIONS = {"ValueError": ValueError, "AssertionError": AssertionError, "IndexError": IndexError, "TypeError": TypeError}


def _raise(L, status: int):
    msg = L.whamd_last_error().decode("utf-8", "replace")
    kind, sep, rest = msg.partition(": ")
    if sep and kind in _EXCEPTIONS:
        raise _EXCEPTIONS[kind](rest)
    raise _native.SolverError(status, msg)


def _as_bytes(s) -> bytes:
    if isinstance(s, bytes):
        return s
    if isinstance(s, (bytearray, memoryview)):
        return bytes(s)
    return str(s).encode()


def _u8(b: bytes) -> np.ndarray:
    return np.frombuffer(b, dtype=np.uint8) if len(b) else np.zeros(1, dtype=np.uint8)


def _csr(chunks: Sequence[bytes]):
    lens = np.fromiter((len(c) for c in chunks), dtype=np.uint64, count=len(chunks))
    ptr = np.zeros(len(chunks) + 1, dtype=np.uint64)
    np.cumsum(lens, out=ptr[1:])
    return ptr, _u8(b"".join(chunks))


class _Variants:
    """The variant list (and the restrictions) as the arrays of whamd_realign_variants_view."""

    def __init__(self, variants, restricted_genotypes=None):
        n = len(variants)
        self.position = np.fromiter((v.position for v in variants), dtype=np.int64, count=n)
        self.ref_ptr, self.ref_bytes = _csr([_as_bytes(v.reference_allele) for v in variants])
        alts = [v.get_alt_allele_list() for v in variants]
        n_alts = np.fromiter((len(a) for a in alts), dtype=np.uint64, count=n)
        self.alt_ptr = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(n_alts, out=self.alt_ptr[1:])
        self.alt_byte_ptr, self.alt_bytes = _csr([_as_bytes(a) for al in alts for a in al])
        self.restrict_ptr = self.restrict_alleles = self.restrict_present = None
        if restricted_genotypes:   # (`if restricted_genotypes` in the reference: an empty list restricts nothing)
            lists, present = [], np.zeros(n, dtype=np.uint8)
            for k in range(n):
                g = restricted_genotypes[k]
                if g is None:
                    lists.append(())
                    continue
                present[k] = 1
                lists.append(tuple(g.as_vector()) if hasattr(g, "as_vector") else tuple(g))
            counts = np.fromiter((len(x) for x in lists), dtype=np.uint64, count=n)
            self.restrict_ptr = np.zeros(n + 1, dtype=np.uint64)
            np.cumsum(counts, out=self.restrict_ptr[1:])
            flat = np.fromiter((a for x in lists for a in x), dtype=np.int64, count=int(counts.sum()))
            self.restrict_alleles = flat if len(flat) else np.zeros(1, dtype=np.int64)
            self.restrict_present = present
        self.view = _native.RealignVariantsView(
            n, _native._ptr(self.position, C.c_int64), _native._ptr(self.ref_ptr, C.c_uint64), _native._ptr(self.ref_bytes, C.c_uint8),
            _native._ptr(self.alt_ptr, C.c_uint64), _native._ptr(self.alt_byte_ptr, C.c_uint64), _native._ptr(self.alt_bytes, C.c_uint8),
            _native._ptr(self.restrict_ptr, C.c_uint64), _native._ptr(self.restrict_alleles, C.c_int64), _native._ptr(self.restrict_present, C.c_uint8))


class _Alignments:
    def __init__(self, alignments, first_variant=None):
        n = len(alignments)
        self.reference_start = np.fromiter((a.reference_start for a in alignments), dtype=np.int64, count=n)
        cigars = [a.cigartuples or () for a in alignments]
        counts = np.fromiter((len(c) for c in cigars), dtype=np.uint64, count=n)
        self.cigar_ptr = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(counts, out=self.cigar_ptr[1:])
        total = int(self.cigar_ptr[-1])
        flat = np.fromiter((x for c in cigars for t in c for x in t), dtype=np.int64, count=2 * total).reshape(total, 2)
        self.cigar_op = np.ascontiguousarray(flat[:, 0], dtype=np.uint32) if total else np.zeros(1, dtype=np.uint32)
        self.cigar_len = np.ascontiguousarray(flat[:, 1], dtype=np.uint32) if total else np.zeros(1, dtype=np.uint32)
        seqs = [a.query_sequence for a in alignments]
        self.seq_present = np.fromiter((s is not None for s in seqs), dtype=np.uint8, count=n)
        self.seq_ptr, self.seq = _csr([b"" if s is None else _as_bytes(s) for s in seqs])
        self.first_variant = None if first_variant is None else np.ascontiguousarray(first_variant, dtype=np.uint64)
        self.view = _native.RealignAlignmentsView(
            n, _native._ptr(self.reference_start, C.c_int64), _native._ptr(self.first_variant, C.c_uint64), _native._ptr(self.cigar_ptr, C.c_uint64),
            _native._ptr(self.cigar_op, C.c_uint32), _native._ptr(self.cigar_len, C.c_uint32), _native._ptr(self.seq_ptr, C.c_uint64),
            _native._ptr(self.seq, C.c_uint8), _native._ptr(self.seq_present, C.c_uint8))


class _Reference:
    def __init__(self, reference, offset: int = 0, chromosome_length: Optional[int] = None):
        b = _as_bytes(reference)
        self.array = _u8(b)
        self.view = _native.RealignReferenceView(_native._ptr(self.array, C.c_uint8), int(offset), len(b),
                                                 int(offset) + len(b) if chromosome_length is None else int(chromosome_length))


def _params(overhang, use_affine, gap_start, gap_extend, default_mismatch) -> _native.RealignParams:
    # gap_start / gap_extend go through Cython `int` parameters (truncated toward zero); mismatch costs are stored as f32.  With one of them
    # None the library raises the reference's assert at the first realigned job (no device pass: the walk fails first).
    unset = bool(use_affine) and (gap_start is None or gap_extend is None or default_mismatch is None)
    ok = bool(use_affine) and not unset
    return _native.RealignParams(int(overhang), 1 if use_affine else 0, int(gap_start) if ok else 1, int(gap_extend) if ok else 1,
                                 float(np.float32(default_mismatch)) if ok else 0.0, 1 if unset else 0)


def detect_alleles_batch(variants, alignments, reference, restricted_genotypes=None, overhang: int = 10, use_affine: bool = False,
                         gap_start=None, gap_extend=None, default_mismatch=None, first_variant=None, device: int = 0,
                         with_stats: bool = False, host: bool = False):
    """detect_alleles_by_alignment for every alignment of a batch in one device round trip: one list of (variant index, allele, quality)
    per alignment, in the order the reference yields them.  first_variant: the ``j`` of every alignment (default 0: the reference skips
    the variants left of the read itself).  reference: the whole chromosome (``str`` or ``bytes``).  host=True runs the debug library's
    host restatement instead of the device (tests only)."""
    L = _native.debug_lib() if host else _native.lib()
    var = _Variants(variants, restricted_genotypes)
    al = _Alignments(alignments, first_variant)
    ref = reference if isinstance(reference, _Reference) else _Reference(reference)
    params = _params(overhang, use_affine, gap_start, gap_extend, default_mismatch)
    h = C.c_void_p()
    if host:
        st = L.whamd_debug_realign_detect_host(C.byref(al.view), C.byref(var.view), C.byref(ref.view), C.byref(params), C.byref(h))
    else:
        st = L.whamd_realign_detect(C.byref(al.view), C.byref(var.view), C.byref(ref.view), C.byref(params), C.c_int(int(device)), C.byref(h))
    if st != _native.WHAMD_OK:
        _raise(L, st)
    try:
        n = int(L.whamd_realign_result_count(h))
        ptr = np.zeros(len(alignments) + 1, dtype=np.uint64)
        vidx = np.zeros(max(n, 1), dtype=np.uint64)
        allele = np.zeros(max(n, 1), dtype=np.int32)
        quality = np.zeros(max(n, 1), dtype=np.int64)
        _native._check(L.whamd_realign_get(h, _native._ptr(ptr, C.c_uint64), _native._ptr(vidx, C.c_uint64), _native._ptr(allele, C.c_int32),
                                           _native._ptr(quality, C.c_int64)), L)
        stats = _native.RealignStats()
        _native._check(L.whamd_realign_get_stats(h, C.byref(stats)), L)
    finally:
        L.whamd_realign_destroy(h)
    triples = list(zip(vidx[:n].tolist(), allele[:n].tolist(), quality[:n].tolist()))
    p = ptr.tolist()
    out = [triples[p[a]:p[a + 1]] for a in range(len(alignments))]
    return (out, stats.as_dict()) if with_stats else out


def detect_alleles_by_alignment(variants, restricted_genotypes, j, bam_read, reference, overhang=10, use_affine=False, gap_start=None,
                                gap_extend=None, default_mismatch=None, use_kmerald=False, kmerald_costs=None, kmer_size=7,
                                kmerald_gappenalty=40, kmerald_window=25, calculated_costs=None, splitted_strings=None, device: int = 0):
    """The staticmethod ReadSetReader.detect_alleles_by_alignment: yields (index, allele, quality) for the variants bam_read covers.
    (An exception is raised before the first yield, where the reference raises it after yielding the earlier decisions.)"""
    if use_kmerald:
        raise NotImplementedError("kmerald realignment (kmer_align) is not implemented on the device")
    yield from detect_alleles_batch(variants, [bam_read], reference, restricted_genotypes, overhang, use_affine, gap_start, gap_extend,
                                    default_mismatch, first_variant=[j], device=device)[0]


def _pairs_arrays(queries, targets):
    qptr, q = _csr([_as_bytes(x) for x in queries])
    tptr, t = _csr([_as_bytes(x) for x in targets])
    return qptr, q, tptr, t


def _distance_call(queries, targets, costs, gap_start, gap_extend, device, host) -> np.ndarray:
    n = len(queries)
    if n != len(targets):
        raise ValueError("as many queries as targets expected")
    out = np.zeros(max(n, 1), dtype=np.int64)
    if n == 0:
        return out[:0]
    qptr, q, tptr, t = _pairs_arrays(queries, targets)
    cost = None
    if costs is not None:
        for k, (qq, cc) in enumerate(zip(queries, costs)):
            if len(qq) != len(cc):
                raise AssertionError()   # assert len(query) == len(mismatch_cost)
        cost = np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=np.float64) for c in costs]) if n else np.zeros(0), dtype=np.float32)
        if len(cost) == 0:
            cost = np.zeros(1, dtype=np.float32)
    L = _native.debug_lib() if host else _native.lib()
    args = (C.c_uint64(n), _native._ptr(qptr, C.c_uint64), _native._ptr(q, C.c_uint8), _native._ptr(tptr, C.c_uint64), _native._ptr(t, C.c_uint8),
            C.c_int(1 if costs is not None else 0), _native._ptr(cost, C.c_float), C.c_int32(int(gap_start)), C.c_int32(int(gap_extend)))
    st = L.whamd_debug_edit_distance_host(*args, _native._ptr(out, C.c_int64)) if host else \
        L.whamd_edit_distance_batch(*args, C.c_int(int(device)), _native._ptr(out, C.c_int64))
    if st != _native.WHAMD_OK:
        _raise(L, st)
    return out[:n]


def debug_long_shape(use_affine: bool, n_long: int, max_target: int) -> dict:
    """TEST INFRASTRUCTURE (debug library, no device): the launch shape of n_long jobs with a query longer than 64 whose longest allele
    window is max_target bytes -- blocks (0: no second launch), block, lds_bytes, scratch_bytes, carry_words, row_floats, global_rows."""
    L = _native.debug_lib()
    shape = _native.DebugRealignShape()
    _native._check(L.whamd_debug_realign_long_shape(C.c_int(1 if use_affine else 0), C.c_uint64(int(n_long)), C.c_uint32(int(max_target)), C.byref(shape)), L)
    return shape.as_dict()


def debug_walk_counts(variants, alignments, reference, restricted_genotypes=None, overhang: int = 10, use_affine: bool = False, gap_start=None,
                      gap_extend=None, default_mismatch=None, first_variant=None) -> dict:
    """TEST INFRASTRUCTURE (debug library, no device): what detect_alleles_batch's host walk counts on these inputs -- n_jobs, n_long (jobs
    with a query longer than 64) and max_target_long (their longest allele window), which decide the second launch."""
    L = _native.debug_lib()
    var = _Variants(variants, restricted_genotypes)
    al = _Alignments(alignments, first_variant)
    ref = reference if isinstance(reference, _Reference) else _Reference(reference)
    params = _params(overhang, use_affine, gap_start, gap_extend, default_mismatch)
    n_jobs, n_long, max_t = C.c_uint64(), C.c_uint64(), C.c_uint32()
    st = L.whamd_debug_realign_walk_counts(C.byref(al.view), C.byref(var.view), C.byref(ref.view), C.byref(params), C.byref(n_jobs), C.byref(n_long),
                                           C.byref(max_t))
    if st != _native.WHAMD_OK:
        _raise(L, st)
    return {"n_jobs": n_jobs.value, "n_long": n_long.value, "max_target_long": max_t.value}


def debug_pair_counts(pairs) -> dict:
    """TEST INFRASTRUCTURE (debug library, no device): n_long and max_target_long of an edit_distance*_batch over these (query, target, ...)."""
    pairs = list(pairs)
    L = _native.debug_lib()
    qptr, _, tptr, _ = _pairs_arrays([p[0] for p in pairs], [p[1] for p in pairs])
    n_long, max_t = C.c_uint64(), C.c_uint32()
    _native._check(L.whamd_debug_edit_distance_long_counts(C.c_uint64(len(pairs)), _native._ptr(qptr, C.c_uint64), _native._ptr(tptr, C.c_uint64),
                                                           C.byref(n_long), C.byref(max_t)), L)
    return {"n_long": n_long.value, "max_target_long": max_t.value}


def edit_distance_batch(pairs, device: int = 0, host: bool = False) -> np.ndarray:
    """edit_distance(s, t) for many (s, t) pairs in one device call."""
    pairs = list(pairs)
    return _distance_call([p[0] for p in pairs], [p[1] for p in pairs], None, 1, 1, device, host)


def edit_distance_affine_gap_batch(triples, gap_start=1, gap_extend=1, device: int = 0, host: bool = False) -> np.ndarray:
    """edit_distance_affine_gap(query, ref, mismatch_cost, gap_start, gap_extend) for many (query, ref, mismatch_cost) triples."""
    triples = list(triples)
    return _distance_call([t[0] for t in triples], [t[1] for t in triples], [t[2] for t in triples], gap_start, gap_extend, device, host)


def edit_distance(s, t, maxdiff: int = -1) -> int:
    """edit_distance(s, t) of whatshap/align.pyx (unbanded only)."""
    if maxdiff != -1:
        raise NotImplementedError("banded edit_distance (maxdiff != -1) is not implemented")
    return int(edit_distance_batch([(s, t)])[0])


def edit_distance_affine_gap(query, ref, mismatch_cost, gap_start=1, gap_extend=1) -> int:
    """edit_distance_affine_gap of whatshap/align.pyx."""
    return int(edit_distance_affine_gap_batch([(query, ref, mismatch_cost)], gap_start, gap_extend)[0])
