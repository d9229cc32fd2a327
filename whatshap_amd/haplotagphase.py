"""Haplotagphase on the device: the compute of ``whatshap haplotagphase`` -- ``compute_votes``, ``consensus``, ``best_candidate`` and
``length_of_homopolymer`` of whatshap/cli/haplotagphase.py (lines 347-395, 203-263, 266-304, 307-344).

Haplotagged reads vote, per variant, for (phase set, haplotype); the consensus picks the key with the largest sum and filters it.  The
native library validates and maps phase sets to dense ids on the host, and counts, scans, places and reduces the votes on the device;
``host=True`` votes on one host thread of the debug library instead (test infrastructure).  All arithmetic is integer, and the one
division is Python's own while the magnitudes stay within 2^53 (beyond, the call refuses): results equal the reference's, ties included.
There is no CPU fallback: without a device the native call raises.

The reference's homopolymer filter can drop nothing: ``length_of_homopolymer`` stops counting at ``threshold`` and the filter asks for a
length above it.  The mirror below keeps both parameters and the function; the device never sees the reference sequence.
"""

from __future__ import annotations

import ctypes as C
import itertools
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _native
from .core import Variant

HOMOZYGOUS, PHASED, SNV = 1, 2, 4   # WHAMD_TAGPHASE_* of include/whatshap_amd.h
NOT_VOTED = np.uint64(0xFFFFFFFFFFFFFFFF)


class TagphaseProblem:
    """One sample on one chromosome, as arrays: per variant a flag byte (HOMOZYGOUS | PHASED | SNV), the reads as a CSR of (variant index,
    id, quality) -- id the index, 0 or 1, of the read's allele in the genotype vector --, per read ``ps`` = PS_tag - 1 and ``hp`` = HP_tag - 1,
    and the two consensus parameters the device applies."""

    def __init__(self, variant_flags, read_ptr, entry_variant, entry_id, entry_quality, read_ps, read_hp, gap_threshold: float = 0.0, only_indels: bool = False):
        self.variant_flags = np.ascontiguousarray(variant_flags, dtype=np.uint8)
        self.read_ptr = np.ascontiguousarray(read_ptr, dtype=np.uint64)
        if self.read_ptr.size == 0:
            self.read_ptr = np.zeros(1, dtype=np.uint64)
        self.n_reads = self.read_ptr.size - 1
        variant = np.asarray(entry_variant, dtype=np.int64)
        if variant.size and (variant.min() < 0 or variant.max() >= 1 << 32):
            raise ValueError("a variant index outside uint32 (out of range)")
        self.entry_variant = np.ascontiguousarray(variant, dtype=np.uint32)
        ids = np.asarray(entry_id, dtype=np.int64)
        self.entry_id = np.ascontiguousarray(np.where((ids == 0) | (ids == 1), ids, 255), dtype=np.uint8)
        quality = np.asarray(entry_quality, dtype=np.int64)
        if quality.size and (quality.min() < -(1 << 31) or quality.max() >= 1 << 31):
            raise ValueError("a quality outside int32")
        self.entry_quality = np.ascontiguousarray(quality, dtype=np.int32)
        n_entries = int(self.read_ptr[-1])
        if not (self.entry_variant.size == self.entry_id.size == self.entry_quality.size == n_entries):
            raise ValueError("entry arrays and read_ptr disagree (mismatched lengths)")
        self.read_ps = np.ascontiguousarray(read_ps, dtype=np.int64)
        self.read_hp = np.ascontiguousarray(read_hp, dtype=np.int32)
        if self.read_ps.size != self.n_reads or self.read_hp.size != self.n_reads:
            raise ValueError("per-read arrays and read_ptr disagree (mismatched lengths)")
        self.gap_threshold = float(gap_threshold)
        self.only_indels = bool(only_indels)

    @classmethod
    def from_reads(cls, is_homozygous: Dict[int, bool], reads, allele_to_id: Dict[int, Dict[int, int]], phased: Optional[dict] = None,
                   change: Optional[dict] = None, gap_threshold: float = 0.0, only_indels: bool = False) -> "TagphaseProblem":
        """From the reference's objects, duck-typed: reads with ``PS_tag``, ``HP_tag`` and iteration over variants with ``position``,
        ``allele``, ``quality``.  The dicts are consulted where the reference consults them: ``is_homozygous[pos]`` for every variant of
        a read that votes, ``allele_to_id[pos][allele]`` where that position is not homozygous (``KeyError`` as there); a read that does
        not vote contributes no entries.  ``problem.positions`` keeps the positions behind the variant indices, in the order met;
        ``problem.missing_phased`` / ``problem.missing_change`` the positions the optional dicts do not have."""
        index: Dict[int, int] = {}
        positions: List[int] = []
        flags: List[int] = []
        read_ptr, evar, eid, equal, rps, rhp = [0], [], [], [], [], []
        for read in reads:
            ps, ht = read.PS_tag - 1, read.HP_tag - 1
            if ht >= 0 and ps >= 0 and ht <= 1:
                for v in read:
                    pos = v.position
                    hom = is_homozygous[pos]
                    at = index.get(pos)
                    if at is None:
                        at = index[pos] = len(positions)
                        positions.append(pos)
                        flags.append(HOMOZYGOUS if hom else 0)
                    ident = 0
                    if not hom:
                        ident = allele_to_id[pos][v.allele]
                        if ident not in (0, 1):
                            raise ValueError(f"position {pos}: allele {v.allele} is number {ident} of the genotype vector; haplotagphase is diploid")
                    evar.append(at)
                    eid.append(ident)
                    equal.append(v.quality)
            read_ptr.append(len(evar))
            rps.append(min(max(ps, -1), (1 << 63) - 1))
            rhp.append(min(max(ht, -1), 2))
        missing_phased, missing_change = set(), set()
        for at, pos in enumerate(positions):
            if phased is not None:
                if pos not in phased:
                    missing_phased.add(pos)
                elif phased[pos] is not None:
                    flags[at] |= PHASED
            if change is not None and only_indels and not flags[at] & (PHASED | HOMOZYGOUS):
                if pos not in change:
                    missing_change.add(pos)
                elif change[pos].is_snv():
                    flags[at] |= SNV
        p = cls(flags, read_ptr, evar, eid, equal, rps, rhp, gap_threshold, only_indels)
        p.positions = positions
        p.missing_phased, p.missing_change = missing_phased, missing_change
        return p

    def view(self, want_table: bool) -> _native.TagphaseView:
        P = _native._ptr
        return _native.TagphaseView(self.variant_flags.size, P(self.variant_flags, C.c_uint8), self.n_reads, P(self.read_ptr, C.c_uint64),
                                    P(self.entry_variant, C.c_uint32), P(self.entry_id, C.c_uint8), P(self.entry_quality, C.c_int32), P(self.read_ps, C.c_int64),
                                    P(self.read_hp, C.c_int32), self.gap_threshold, 1 if self.only_indels else 0, 1 if want_table else 0)


class TagphaseResult:
    """Per variant ``voted``, ``first`` (index of its first voting entry; orders the reference's dicts), ``n_phasesets``, ``best_ps``,
    ``best_id``, ``score``, ``total``, ``kept``, ``zero_total``; ``n_skipped``; with ``want_table`` the vote table as ``row_ptr`` and per
    row ``row_ps``, ``row_sum0``, ``row_sum1``, ``row_first`` (a variant's rows ascend in ``row_first``); ``stats``."""

    FIELDS = ("voted", "first", "n_phasesets", "best_ps", "best_id", "score", "total", "kept", "zero_total")
    TABLE_FIELDS = ("row_ptr", "row_ps", "row_sum0", "row_sum1", "row_first")

    def __init__(self, fields, table, stats):
        for name, value in zip(self.FIELDS, fields):
            setattr(self, name, value)
        for name, value in zip(self.TABLE_FIELDS, table or (None,) * 5):
            setattr(self, name, value)
        self.stats = stats
        self.n_skipped = int(stats["n_skipped"])

    def order(self) -> np.ndarray:
        """The voted variants in the order the reference's ``votes`` dict holds them."""
        voted = np.flatnonzero(self.voted)
        return voted[np.argsort(self.first[voted], kind="stable")]


def tagphase_batch(problems: Sequence[TagphaseProblem], device: int = 0, host: bool = False, want_table: Union[bool, Sequence[bool]] = False,
                   stats: Optional[list] = None) -> List[TagphaseResult]:
    """Every problem (chromosome x sample) in one native call: one upload, 7 launches (11 with ``want_table``) whatever the problems.
    ``want_table`` is one flag for all problems or one per problem.
    ``stats``, if given, receives one dict per problem (its counts; launches and times are those of the whole call)."""
    P = _native._ptr
    wants = [want_table] * len(problems) if isinstance(want_table, bool) else list(want_table)
    with _native.batch_handle(host, [p.view(w) for p, w in zip(problems, wants)], "whamd_tagphase", "whamd_debug_tagphase_host", "whamd_tagphase_destroy",
                              device=device) as (L, h):
        out = []
        for k in range(len(problems)):
            cnt = L.whamd_tagphase_count(h, k)
            u8 = lambda: np.zeros(cnt, dtype=np.uint8)   # noqa: E731
            i64 = lambda: np.zeros(cnt, dtype=np.int64)   # noqa: E731
            voted, first, nps, best_ps, best_id, score, total, kept, zero = u8(), np.zeros(cnt, dtype=np.uint64), np.zeros(cnt, dtype=np.uint32), i64(), u8(), i64(), i64(), u8(), u8()
            _native.checked(L, L.whamd_tagphase_get(h, k, P(voted, C.c_uint8), P(first, C.c_uint64), P(nps, C.c_uint32), P(best_ps, C.c_int64),
                                                    P(best_id, C.c_uint8), P(score, C.c_int64), P(total, C.c_int64), P(kept, C.c_uint8), P(zero, C.c_uint8)))
            table = None
            if wants[k]:
                rows = L.whamd_tagphase_row_count(h, k)
                table = (np.zeros(cnt + 1, dtype=np.uint64), np.zeros(rows, dtype=np.int64), np.zeros(rows, dtype=np.int64), np.zeros(rows, dtype=np.int64),
                         np.zeros(rows, dtype=np.uint64))
                _native.checked(L, L.whamd_tagphase_get_table(h, k, P(table[0], C.c_uint64), P(table[1], C.c_int64), P(table[2], C.c_int64),
                                                              P(table[3], C.c_int64), P(table[4], C.c_uint64)))
            ts = _native.read_stats(L, "whamd_tagphase_get_stats", _native.TagphaseStats, h, k)
            out.append(TagphaseResult((voted, first, nps, best_ps, best_id, score, total, kept, zero), table, ts))
            if stats is not None:
                stats.append(dict(ts))
        return out


# ---------------------------------------------------------------------------------------------- the reference's signatures
def compute_votes(is_homozygous: Dict[int, bool], reads, allele_to_id: Dict[int, Dict[int, int]], *, device: int = 0, host: bool = False,
                  stats: Optional[list] = None, skipped: Optional[list] = None) -> Dict[int, Dict[Tuple[int, int], int]]:
    """compute_votes (haplotagphase.py:347-395): the same nested dict -- keys, key order and values.  ``skipped``, if given, receives the
    number of reads the reference's warning counts.  It never raises for a zero total."""
    problem = TagphaseProblem.from_reads(is_homozygous, reads, allele_to_id)
    res = tagphase_batch([problem], device=device, host=host, want_table=True, stats=stats)[0]
    if skipped is not None:
        skipped.append(res.n_skipped)
    votes: Dict[int, Dict[Tuple[int, int], int]] = {}
    for x in res.order().tolist():
        vote = votes[problem.positions[x]] = {}
        for row in range(int(res.row_ptr[x]), int(res.row_ptr[x + 1])):
            ps = int(res.row_ps[row])
            vote[(ps, 0)] = int(res.row_sum0[row])
            vote[(ps, 1)] = int(res.row_sum1[row])
    return votes


def best_candidate(var: Dict[Tuple[int, int], int]) -> Tuple[int, int, float, int]:
    """best_candidate (haplotagphase.py:266-304): (allele, phase set, score / total, score) of the largest value, the first inserted among
    equals.  ``ZeroDivisionError`` at a zero total, as there."""
    best_key, score, total = None, 0, 0
    for key, value in var.items():
        total += value
        if best_key is None or value > score:
            best_key, score = key, value
    if best_key is None:
        raise IndexError("list index out of range")   # (the reference's lst[0])
    phase_set, allele = best_key
    return allele, phase_set, score / total, score


def length_of_homopolymer(ref: str, start: int, step: int, threshold: int) -> int:
    """length_of_homopolymer (haplotagphase.py:307-344): equal characters from ``start`` in steps of ``step``, never more than ``threshold``."""
    res = 0
    for i in itertools.count(start, step):
        if res < threshold and 0 <= i < len(ref) and ref[i] == ref[start]:
            res += 1
        else:
            break
    return res


def _filtered(pos, fraction, only_indels, gap_threshold, cut_homopolymers, refseq, change) -> bool:
    if 100 * fraction < gap_threshold:
        return True
    if only_indels and change[pos].is_snv():
        return True
    if cut_homopolymers > 0:   # (inert: the length is capped at the threshold it would have to exceed)
        longest = max(length_of_homopolymer(refseq, pos + 1, 1, cut_homopolymers), length_of_homopolymer(refseq, pos, -1, cut_homopolymers))
        if longest > cut_homopolymers:
            return True
    return False


def consensus(only_indels: bool, gap_threshold, cut_homopolymers: int, refseq: str, change: dict, phased: dict, votes: Dict[int, Dict[Tuple[int, int], int]],
              id_to_allele: Dict[int, Dict[int, int]]):
    """consensus (haplotagphase.py:203-263) on a votes dict: (super_reads, components).  Plain Python -- a caller that wants votes and
    consensus in one device call uses :func:`votes_and_consensus`."""
    super_reads: List[List[Variant]] = [[], []]
    components: Dict[int, int] = {}
    for pos, vote in votes.items():
        best_allele, phase_set, fraction, score = best_candidate(vote)
        components[pos] = phase_set
        if phased[pos] is None and _filtered(pos, fraction, only_indels, gap_threshold, cut_homopolymers, refseq, change):
            continue
        super_reads[0].append(Variant(pos, id_to_allele[pos][best_allele], score))
        super_reads[1].append(Variant(pos, id_to_allele[pos][1 - best_allele], score))
    for read in super_reads:
        read.sort(key=lambda x: x.position)
    return super_reads, components


def votes_and_consensus(is_homozygous: Dict[int, bool], reads, allele_to_id: Dict[int, Dict[int, int]], only_indels: bool, gap_threshold, cut_homopolymers: int,
                        refseq: str, change: dict, phased: dict, id_to_allele: Dict[int, Dict[int, int]], *, device: int = 0, host: bool = False,
                        stats: Optional[list] = None):
    """compute_votes followed by consensus, as run_haplotagphase calls them, in one device call and without the vote table:
    ((super_reads, components), number_of_skipped).  Raises what the pair raises: ``KeyError`` for a position or allele the dicts lack,
    ``ZeroDivisionError`` for a voted position whose sums add up to zero."""
    problem = TagphaseProblem.from_reads(is_homozygous, reads, allele_to_id, phased, change, gap_threshold, only_indels)
    res = tagphase_batch([problem], device=device, host=host, stats=stats)[0]
    super_reads: List[List[Variant]] = [[], []]
    components: Dict[int, int] = {}
    for x in res.order().tolist():
        pos = problem.positions[x]
        if res.zero_total[x]:
            raise ZeroDivisionError("division by zero")
        components[pos] = int(res.best_ps[x])
        if pos in problem.missing_phased:
            raise KeyError(pos)
        if not res.kept[x]:
            continue
        if pos in problem.missing_change:   # (it passed the gap threshold: the reference asks change[pos] now)
            raise KeyError(pos)
        best, score = int(res.best_id[x]), int(res.score[x])
        super_reads[0].append(Variant(pos, id_to_allele[pos][best], score))
        super_reads[1].append(Variant(pos, id_to_allele[pos][1 - best], score))
    for read in super_reads:
        read.sort(key=lambda v: v.position)
    return (super_reads, components), res.n_skipped
