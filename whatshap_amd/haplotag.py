"""Haplotagging on the device: the assignment step of ``whatshap haplotag`` -- ``prepare_haplotag_information``,
``get_variant_information`` and ``read_representation`` of whatshap/cli/haplotag.py (lines 322-427, 133-153, 288-304).

Every read, or group of linked reads, goes to the phase set and the haplotype its alleles support best.  The native library forms the
groups on the host (the sequential part) and scores them on the device; ``host=True`` scores them on one host thread of the debug
library instead (test infrastructure).  All arithmetic is integer: results equal the reference's, ties included.  There is no CPU
fallback: without a device the native call raises.

Where the reference is not a function of its input: its ``reads_to_consider`` is a ``set`` of reads, so the order in which a group of
several linked reads first meets its phase sets -- which decides a tie between two phase sets on the largest haplotype sum, and nothing
else -- is arbitrary there.  Here it is defined: the seed first, then the other members in read-set order, each read's variants as listed.
A phase set counts as met once an allele of the read equals the allele of one of its haplotypes (the reference creates the phase set's
cost row at that moment).
"""

from __future__ import annotations

import ctypes as C
from collections import defaultdict
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np

from . import _native

PRIMARY_DEFAULT_SUB_ALIGNMENT_ID = "____1"   # whatshap/variants.py
MAX_PLOIDY = 16
NO_BX = 0xFFFFFFFF


@dataclass(frozen=True)
class ReadAlignmentRepresentation:
    read_name: str
    chromosome: str
    is_supplementary: bool
    sub_alignment_id: str


@dataclass(frozen=True)
class PrimaryInfo:
    reference_start: int
    reference_end: int
    is_reverse: bool


def read_representation(read, as_primary: bool = False) -> ReadAlignmentRepresentation:
    """read_representation (haplotag.py:288-304): the key under which a read is processed and assigned.  As there, the name loses a
    suffix equal to the representation's sub-alignment id, and what is cut off has the length of the read's own id."""
    sub_alignment_id = PRIMARY_DEFAULT_SUB_ALIGNMENT_ID if as_primary else read.sub_alignment_id
    read_name = read.name
    if read_name.endswith(sub_alignment_id):
        read_name = read_name[: -len(read.sub_alignment_id)]
    return ReadAlignmentRepresentation(read_name=read_name, chromosome=read.chromosome, is_supplementary=False if as_primary else read.is_supplementary,
                                       sub_alignment_id=sub_alignment_id)


def get_variant_information(variant_table, sample):
    """What get_variant_information (haplotag.py:133-153) returns for one sample: a dict position -> (phase set as int, phasing tuple) over
    the variants that are phased and have a phase set, and the list of those among them whose genotype is not homozygous (what the reader
    is asked to detect alleles at).  ``variant_table`` is duck-typed: ``variants``, ``genotypes_of(sample)``, ``phases_of(sample)``."""
    table_variants = list(variant_table.variants)
    calls = variant_table.phases_of(sample)
    genotypes = variant_table.genotypes_of(sample)
    phased = [k for k in range(min(len(table_variants), len(genotypes), len(calls))) if calls[k] is not None and calls[k].block_id is not None]
    phase_info = {table_variants[k].position: (int(calls[k].block_id), calls[k].phase) for k in phased}
    heterozygous = [table_variants[k] for k in phased if not genotypes[k].is_homozygous()]
    return phase_info, heterozygous


def _check_ploidy(ploidy) -> int:
    ploidy = int(ploidy)
    if ploidy < 2:
        raise ValueError(f"ploidy {ploidy} below 2: there is no second-best haplotype (the reference raises IndexError)")
    if ploidy > MAX_PLOIDY:
        raise ValueError(f"ploidy {ploidy} above the limit of {MAX_PLOIDY}")
    return ploidy


class HaplotagProblem:
    """One sample on one chromosome, as arrays: the phased variants (position, phase set, phasing [n_variants][ploidy]), the reads as a
    CSR of (position, allele, quality), and per read its start, the dense id of its representation and of its BX tag (NO_BX: none)."""

    def __init__(self, ploidy: int, variant_position, variant_phaseset, variant_phasing, read_ptr, entry_position, entry_allele, entry_quality, read_start,
                 read_repr, read_bx=None, linked_reads: bool = True, linked_read_cutoff: int = 50000):
        self.ploidy = _check_ploidy(ploidy)
        self.variant_position = np.ascontiguousarray(variant_position, dtype=np.int64)
        self.variant_phaseset = np.ascontiguousarray(variant_phaseset, dtype=np.int64)
        phasing = np.asarray(variant_phasing, dtype=np.int64).reshape(-1, self.ploidy) if np.size(variant_phasing) else np.zeros((0, self.ploidy), dtype=np.int64)
        self.variant_phasing = np.ascontiguousarray(np.where((phasing == 0) | (phasing == 1), phasing, -1), dtype=np.int8)
        if not (self.variant_position.size == self.variant_phaseset.size == self.variant_phasing.shape[0]):
            raise ValueError("variant arrays differ in length (mismatched lengths)")
        self.read_ptr = np.ascontiguousarray(read_ptr, dtype=np.uint64)
        if self.read_ptr.size == 0:
            self.read_ptr = np.zeros(1, dtype=np.uint64)
        self.n_reads = self.read_ptr.size - 1
        self.entry_position = np.ascontiguousarray(entry_position, dtype=np.int64)
        allele = np.asarray(entry_allele, dtype=np.int64)
        self.entry_allele = np.ascontiguousarray(np.where((allele == 0) | (allele == 1), allele, np.clip(allele, -128, 127)), dtype=np.int8)
        quality = np.asarray(entry_quality, dtype=np.int64)
        if quality.size and (quality.min() < -(1 << 31) or quality.max() >= 1 << 31):
            raise ValueError("a quality outside int32")
        self.entry_quality = np.ascontiguousarray(quality, dtype=np.int32)
        n_entries = int(self.read_ptr[-1])
        if not (self.entry_position.size == self.entry_allele.size == self.entry_quality.size == n_entries):
            raise ValueError("entry arrays and read_ptr disagree (mismatched lengths)")
        self.read_start = np.ascontiguousarray(read_start, dtype=np.int64)
        self.read_repr = np.ascontiguousarray(read_repr, dtype=np.uint32)
        self.read_bx = None if read_bx is None else np.ascontiguousarray(read_bx, dtype=np.uint32)
        if self.read_start.size != self.n_reads or self.read_repr.size != self.n_reads or (self.read_bx is not None and self.read_bx.size != self.n_reads):
            raise ValueError("per-read arrays and read_ptr disagree (mismatched lengths)")
        self.linked_reads = bool(linked_reads)
        self.linked_read_cutoff = int(linked_read_cutoff)
        if not -(1 << 63) <= self.linked_read_cutoff < 1 << 63:
            raise ValueError("linked_read_cutoff outside int64")

    @classmethod
    def from_reads(cls, variantpos_to_phaseinfo: Dict[int, tuple], read_set, ploidy: int, ignore_linked_read: bool, linked_read_cutoff: int,
                   representation: Callable = read_representation) -> "HaplotagProblem":
        """From the reference's objects, duck-typed: the map of get_variant_information and a read set (``name``, ``chromosome``,
        ``sub_alignment_id``, ``is_supplementary``, ``reference_start``, ``BX_tag`` / ``has_BX_tag()``, iteration over variants with
        ``position``, ``allele``, ``quality``).  ``problem.reads`` / ``problem.reprs`` / ``problem.bx_tags`` keep the objects behind the ids."""
        ploidy = _check_ploidy(ploidy)
        positions = list(variantpos_to_phaseinfo)
        phasesets, phasing = [], []
        for pos in positions:
            block_id, phase = variantpos_to_phaseinfo[pos]
            phase = tuple(phase)
            if len(phase) != ploidy:
                raise ValueError(f"position {pos}: phasing of {len(phase)} alleles at ploidy {ploidy} (mismatched lengths)")
            phasesets.append(int(block_id))
            phasing.append([a if a in (0, 1) else -1 for a in phase])
        reads = list(read_set)
        repr_ids: Dict[object, int] = {}
        bx_ids: Dict[object, int] = {}
        read_ptr, epos, eall, equal, start, rrepr, rbx = [0], [], [], [], [], [], []
        for read in reads:
            for v in read:
                epos.append(v.position)
                eall.append(v.allele)
                equal.append(v.quality)
            read_ptr.append(len(epos))
            start.append(read.reference_start)
            rrepr.append(repr_ids.setdefault(representation(read, False), len(repr_ids)))
            rbx.append(bx_ids.setdefault(read.BX_tag, len(bx_ids)) if not ignore_linked_read and read.has_BX_tag() else NO_BX)
        p = cls(ploidy, positions, phasesets, phasing, read_ptr, epos, eall, equal, start, rrepr, rbx, not ignore_linked_read, linked_read_cutoff)
        p.reads = reads
        p.reprs = list(repr_ids)
        p.bx_tags = list(bx_ids)
        return p

    def view(self) -> _native.HaplotagView:
        P = _native._ptr
        return _native.HaplotagView(self.ploidy, 1 if self.linked_reads else 0, self.linked_read_cutoff, self.variant_position.size,
                                    P(self.variant_position, C.c_int64), P(self.variant_phaseset, C.c_int64), P(self.variant_phasing, C.c_int8), self.n_reads,
                                    P(self.read_ptr, C.c_uint64), P(self.entry_position, C.c_int64), P(self.entry_allele, C.c_int8),
                                    P(self.entry_quality, C.c_int32), P(self.read_start, C.c_int64), P(self.read_repr, C.c_uint32), P(self.read_bx, C.c_uint32))


class HaplotagResult:
    """Per read ``haplotype`` (-1: none), ``quality``, ``phaseset``; the assigned linked-read groups in processing order as
    ``bx`` (tag id), ``bx_start``, ``bx_haplotype``, ``bx_phaseset``; ``n_multiple_phase_sets``; ``stats``."""

    def __init__(self, haplotype, quality, phaseset, bx, bx_start, bx_haplotype, bx_phaseset, stats):
        self.haplotype, self.quality, self.phaseset = haplotype, quality, phaseset
        self.bx, self.bx_start, self.bx_haplotype, self.bx_phaseset = bx, bx_start, bx_haplotype, bx_phaseset
        self.stats = stats
        self.n_multiple_phase_sets = int(stats["n_multiple_phase_sets"])


def haplotag_batch(problems: Sequence[HaplotagProblem], device: int = 0, host: bool = False, stats: Optional[list] = None) -> List[HaplotagResult]:
    """Every problem (chromosome x sample) in one native call: one upload, at most three launches, one download for the whole batch.
    ``stats``, if given, receives one dict per problem (its counts; launches and times are those of the whole call)."""
    with _native.batch_handle(host, [p.view() for p in problems], "whamd_haplotag", "whamd_debug_haplotag_host", "whamd_haplotag_destroy",
                              device=device) as (L, h):
        out = []
        for k in range(len(problems)):
            cnt = L.whamd_haplotag_count(h, k)
            hap = np.empty(cnt, dtype=np.int32)
            qual = np.empty(cnt, dtype=np.int64)
            ps = np.empty(cnt, dtype=np.int64)
            if cnt:
                _native.checked(L, L.whamd_haplotag_get(h, k, _native._ptr(hap, C.c_int32), _native._ptr(qual, C.c_int64), _native._ptr(ps, C.c_int64)))
            nbx = L.whamd_haplotag_bx_count(h, k)
            bx = np.empty(nbx, dtype=np.uint32)
            bx_start = np.empty(nbx, dtype=np.int64)
            bx_hap = np.empty(nbx, dtype=np.int32)
            bx_ps = np.empty(nbx, dtype=np.int64)
            if nbx:
                _native.checked(L, L.whamd_haplotag_get_bx(h, k, _native._ptr(bx, C.c_uint32), _native._ptr(bx_start, C.c_int64), _native._ptr(bx_hap, C.c_int32),
                                                           _native._ptr(bx_ps, C.c_int64)))
            hs = _native.read_stats(L, "whamd_haplotag_get_stats", _native.HaplotagStats, h, k)
            out.append(HaplotagResult(hap, qual, ps, bx, bx_start, bx_hap, bx_ps, hs))
            if stats is not None:
                stats.append(dict(hs))
        return out


def prepare_haplotag_information(variant_table, shared_samples, phased_input_reader, regions, ignore_linked_read, linked_read_cutoff, ploidy,
                                 supplementary_strategy=None, *,
                                 representation: Callable = read_representation, device: int = 0, host: bool = False, stats: Optional[list] = None):
    """whatshap.cli.haplotag.prepare_haplotag_information (haplotag.py:322-427): (BX_tag_to_haplotype, read_to_haplotype,
    n_multiple_phase_sets, primary_info_by_repr).  Results are keyed by this module's ReadAlignmentRepresentation; a caller inside WhatsHap
    passes ``representation=whatshap.cli.haplotag.read_representation`` to get the reference's own key type.  As in the reference, a later
    sample overwrites an earlier one's entries, reads are marked processed per sample, and ``supplementary_strategy`` (any value, the
    reference's enum included) is accepted and not consulted.

    Two differences to the reference.  Every read is validated before anything is scored, also a read the reference would skip because
    its representation was processed already: an unknown position or an allele outside {0, 1} in such a read raises ``ValueError`` here
    and passes there.  And this entry point still walks every (read, variant) pair once in the interpreter to turn the duck-typed objects
    into arrays -- the haplotype loop, the grouping and the selection run natively, the object walk does not; a caller that has arrays
    uses :func:`haplotag_batch`, which has no per-read Python work."""
    ploidy = _check_ploidy(ploidy)
    n_multiple_phase_sets = 0
    BX_tag_to_haplotype = defaultdict(list)
    read_to_haplotype = {}
    primary_info_by_repr = {}
    for sample in shared_samples:
        variantpos_to_phaseinfo, variants = get_variant_information(variant_table, sample)
        read_set, _ = phased_input_reader.read(variant_table.chromosome, variants, sample, regions=regions)
        problem = HaplotagProblem.from_reads(variantpos_to_phaseinfo, read_set, ploidy, ignore_linked_read, linked_read_cutoff, representation)
        for read in problem.reads:
            if not read.is_supplementary:
                primary_info_by_repr[representation(read, True)] = PrimaryInfo(reference_start=read.reference_start, reference_end=read.reference_end,
                                                                               is_reverse=read.is_reverse)
        result = haplotag_batch([problem], device=device, host=host, stats=stats)[0]
        n_multiple_phase_sets += result.n_multiple_phase_sets
        for k in range(result.bx.size):
            BX_tag_to_haplotype[problem.bx_tags[int(result.bx[k])]].append((int(result.bx_start[k]), int(result.bx_haplotype[k]), int(result.bx_phaseset[k])))
        for r in np.flatnonzero(result.haplotype >= 0).tolist():
            read_to_haplotype[problem.reprs[int(problem.read_repr[r])]] = (int(result.haplotype[r]), int(result.quality[r]), int(result.phaseset[r]))
    return BX_tag_to_haplotype, read_to_haplotype, n_multiple_phase_sets, primary_info_by_repr
