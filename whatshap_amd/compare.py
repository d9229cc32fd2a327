"""Comparing polyploid phasings on the device: ``compare_block``, ``compute_switch_errors_poly`` and ``compute_switch_flips_poly`` of
``whatshap compare`` (whatshap/cli/compare.py) and the ``SwitchFlipCalculator`` behind them (src/polyphase/switchflipcalculator.cpp).

A job is two phasings of the same positions and two costs; the program is a Viterbi pass over the ploidy! permutations of the haplotypes
per visited position (one workgroup per job, any number of jobs in one launch).  ``host=True`` runs the same inline functions in the
debug library on one host thread instead (test infrastructure, bit-identical to the device).  There is no CPU fallback: without a device
the native library raises.

Identical to the reference: the total cost, the minimum Hamming distance, ``diff_genotypes`` and the matching positions, the switch-error
count (flip cost ``2 * num_vars * ploidy + 1``: no flip is chosen and the count is unique), the result for exactly one position --
``switches = ploidy - 1`` before the division, because the reference's backtrace start counts the differences to ``Permutation::INVALID``
without a guard for position 0 -- and the early returns of ``compute_switch_flips_poly_bt``.

Defined here, because the reference's answer is an artefact of hash order (among equal candidates it takes the first in the iteration
order of a ``std::unordered_map``): among the paths of minimum total cost the one with the fewest flips; among those, the predecessor of
lowest lexicographic rank at every step and the end state of lowest rank.  Rank is the order of ``std::next_permutation`` from the
identity, which is the order of ``itertools.permutations(range(ploidy))``.  Under this rule ``switches`` and ``flips`` depend on the input
alone; the reference never has fewer flips.  libstdc++'s hash table is not emulated.

Phasings are given as the reference takes them, one string or sequence per haplotype, over the digits 0-9 or ints up to 255.
"""

from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native


class SwitchFlips:
    """compare.SwitchFlips."""

    def __init__(self, switches=0, flips=0):
        self.switches = switches
        self.flips = flips

    def __iadd__(self, other):
        self.switches += other.switches
        self.flips += other.flips
        return self

    def __repr__(self):
        return f"SwitchFlips(switches={self.switches}, flips={self.flips})"

    def __str__(self):
        return f"{self.switches}/{self.flips}"


class PhasingErrors:
    """compare.PhasingErrors."""

    def __init__(self, switches=0, hamming=0, switch_flips: Optional[SwitchFlips] = None, diff_genotypes=0):
        self.switches = switches
        self.hamming = hamming
        self.switch_flips = SwitchFlips() if switch_flips is None else switch_flips
        self.diff_genotypes = diff_genotypes

    def __iadd__(self, other):
        if not isinstance(other, PhasingErrors):
            raise TypeError("Can only add to PhasingErrors")
        self.switches += other.switches
        self.hamming += other.hamming
        self.switch_flips += other.switch_flips
        self.diff_genotypes += other.diff_genotypes
        return self

    def __repr__(self):
        return "PhasingErrors(switches={}, hamming={}, switch_flips={}, diff_genotypes={})".format(self.switches, self.hamming, self.switch_flips,
                                                                                                  self.diff_genotypes)


def phasing_array(phasing) -> np.ndarray:
    """One string or sequence per haplotype -> uint8 [n_pos][ploidy], position-major (an array of that shape and type passes through)."""
    if isinstance(phasing, np.ndarray) and phasing.dtype == np.uint8 and phasing.ndim == 2:
        return np.ascontiguousarray(phasing)
    rows = []
    for hap in phasing:
        if isinstance(hap, str):
            row = np.frombuffer(hap.encode("ascii"), dtype=np.uint8).astype(np.int64) - ord("0")
            if row.size and (row.min() < 0 or row.max() > 9):
                raise ValueError("a phasing string holds a character outside 0-9")
        else:
            row = np.asarray([int(a) for a in hap], dtype=np.int64)
            if row.size and (row.min() < 0 or row.max() > 255):
                raise ValueError("allele outside [0, 255]")
        rows.append(row)
    if len({len(r) for r in rows}) > 1:
        raise ValueError("haplotypes of one phasing differ in length")
    if not rows:
        return np.zeros((0, 0), dtype=np.uint8)
    return np.ascontiguousarray(np.stack(rows, axis=1), dtype=np.uint8)


class CompareJob:
    """One job of :func:`switch_flips_batch`: the arrays behind a ``whamd_poly_compare_view``.  ``phasing0`` / ``phasing1``: what
    :func:`phasing_array` takes."""

    def __init__(self, phasing0, phasing1, switch_cost=1.0, flip_cost=1.0, matched_only: bool = False, want_path: bool = False):
        self.phasing0, self.phasing1 = phasing_array(phasing0), phasing_array(phasing1)
        if self.phasing0.shape != self.phasing1.shape:
            raise ValueError(f"the phasings differ in shape: {self.phasing0.shape[::-1]} and {self.phasing1.shape[::-1]} (haplotypes, positions)")
        self.n_pos, self.ploidy = self.phasing0.shape
        self.switch_cost, self.flip_cost = float(switch_cost), float(flip_cost)
        self.matched_only, self.want_path = bool(matched_only), bool(want_path)

    def view(self) -> _native.PolyCompareView:
        p = _native._ptr
        return _native.PolyCompareView(self.ploidy, int(self.matched_only), self.n_pos, p(self.phasing0, C.c_uint8), p(self.phasing1, C.c_uint8),
                                       self.switch_cost, self.flip_cost, int(self.want_path), 0)


class CompareResult:
    """What one job returns.  ``total``: the program's minimum; ``switches`` / ``flips``: raw counts, not divided by the ploidy;
    ``n_matched``; ``n_visited``; ``min_hamming_sum``: min over permutations of the disagreements summed over the visited positions.
    With ``want_path``, per visited position and front to back: ``positions``, ``ranks``, ``perms`` [..][ploidy], ``flipped`` [..][ploidy]
    (1 where phasing0[perm[i]] != phasing1[i]) and ``switches_in_column``; else None."""

    def __init__(self, res, path=None):
        self.total, self.switches, self.flips = float(res.total), int(res.switches), int(res.flips)
        self.n_matched, self.n_visited, self.min_hamming_sum = int(res.n_matched), int(res.n_visited), int(res.min_hamming_sum)
        self.positions, self.ranks, self.perms, self.flipped, self.switches_in_column = path if path is not None else (None,) * 5


def switch_flips_batch(jobs: Sequence[CompareJob], device: int = 0, host: bool = False, stats: Optional[list] = None) -> List[CompareResult]:
    """Every job in one native call (one upload, at most two launches, one download for the whole batch).  ``stats``, if given,
    receives one dict for the call (counts, launches and timings)."""
    p = _native._ptr
    with _native.batch_handle(host, [job.view() for job in jobs], "whamd_poly_compare", "whamd_debug_poly_compare_host", "whamd_poly_compare_destroy",
                              device=device) as (L, h):
        res = (_native.PolyCompareJobResult * max(len(jobs), 1))()
        _native.checked(L, L.whamd_poly_compare_get(h, res))
        out = []
        for x, job in enumerate(jobs):
            path = None
            if job.want_path:
                m = L.whamd_poly_compare_path_count(h, x)
                positions, ranks = np.empty(m, dtype=np.uint64), np.empty(m, dtype=np.uint16)
                perms, flipped = np.empty((m, job.ploidy), dtype=np.uint8), np.empty((m, job.ploidy), dtype=np.uint8)
                switches = np.empty(m, dtype=np.uint32)
                _native.checked(L, L.whamd_poly_compare_get_path(h, x, p(positions, C.c_uint64), p(ranks, C.c_uint16), p(perms, C.c_uint8),
                                                                 p(flipped, C.c_uint8), p(switches, C.c_uint32)))
                path = (positions, ranks, perms, flipped, switches)
            out.append(CompareResult(res[x], path))
        if stats is not None:
            stats.append(_native.read_stats(L, "whamd_poly_compare_get_stats", _native.PolyCompareStats, h))
        return out


# ---------------------------------------------------------------------------------------------- blocks
def _diploid_block(p0: np.ndarray, p1: np.ndarray, n_matched: int) -> PhasingErrors:
    """compare_block's branch for ploidy 2 (host arithmetic on the first haplotype of each phasing, as in the reference)."""
    a, b = p0[:, 0].astype(np.int64), p1[:, 0].astype(np.int64)
    # where one phasing changes allele between neighbours and the other does not
    disagree = ((a[1:] != a[:-1]) != (b[1:] != b[:-1])).tolist()
    result = SwitchFlips()
    run = 0
    for d in disagree + [False]:   # a run of r disagreements in a row is r // 2 flips and r % 2 switches
        if d:
            run += 1
        else:
            result.flips += run // 2
            result.switches += run % 2
            run = 0
    straight = int((p0 != p1).sum())
    crossed = int((p0[:, ::-1] != p1).sum())
    return PhasingErrors(switches=int(sum(disagree)), hamming=int(min(straight, crossed) / 2.0), switch_flips=result, diff_genotypes=len(a) - n_matched)


def _matching_positions(p0: np.ndarray, p1: np.ndarray) -> np.ndarray:
    return np.flatnonzero((np.sort(p0, axis=1) == np.sort(p1, axis=1)).all(axis=1))


def compare_blocks(blocks: Sequence[Tuple], device: int = 0, host: bool = False, stats: Optional[list] = None) -> List[PhasingErrors]:
    """compare.compare_block for every (phasing0, phasing1) of ``blocks``, in one native call: a block above ploidy 2 is two jobs -- all
    positions with costs (1, 1), which also yields the Hamming minimum, and the matching positions with switch cost 1 and flip cost
    ``2 * num_vars * ploidy + 1`` (num_vars: the unfiltered block length, as in the reference).  Blocks of ploidy 2 take the reference's
    diploid branch on the host."""
    arrays = []
    for phasing0, phasing1 in blocks:
        p0, p1 = phasing_array(phasing0), phasing_array(phasing1)
        if p0.shape != p1.shape:
            raise ValueError(f"the phasings differ in shape: {p0.shape[::-1]} and {p1.shape[::-1]} (haplotypes, positions)")
        if p0.shape[1] < 2:
            raise ValueError(f"ploidy {p0.shape[1]} below 2")
        arrays.append((p0, p1))
    jobs, first = [], []
    for p0, p1 in arrays:
        n, k = p0.shape
        first.append(len(jobs))
        if k > 2:
            jobs.append(CompareJob(p0, p1, 1.0, 1.0))
            jobs.append(CompareJob(p0, p1, 1.0, float(2 * n * k + 1), matched_only=True))
    res = switch_flips_batch(jobs, device=device, host=host, stats=stats) if jobs else []
    out = []
    for (p0, p1), at in zip(arrays, first):
        n, k = p0.shape
        if k == 2:
            out.append(_diploid_block(p0, p1, len(_matching_positions(p0, p1))))
            continue
        both, matched = res[at], res[at + 1]
        assert matched.flips == 0
        out.append(PhasingErrors(switches=matched.switches / k, hamming=both.min_hamming_sum / float(k),
                                 switch_flips=SwitchFlips(both.switches / k, both.flips / k), diff_genotypes=n - both.n_matched))
    return out


# ---------------------------------------------------------------------------------------------- the reference's signatures
def compute_matching_genotype_pos(phasing0, phasing1) -> List[int]:
    """compare.compute_matching_genotype_pos: the positions at which both phasings hold the same multiset of alleles (host arithmetic;
    the native call recognises them itself)."""
    assert len(phasing0) == len(phasing1)
    assert len(phasing0) >= 2
    p0, p1 = phasing_array(phasing0), phasing_array(phasing1)
    assert p0.shape == p1.shape
    return _matching_positions(p0, p1).tolist()


def compute_switch_flips_poly_bt(phasing0, phasing1, report_error_positions=False, switch_cost=1, flip_cost=1, device: int = 0, host: bool = False):
    """compare.compute_switch_flips_poly_bt: (SwitchFlips with switches / ploidy and flips / ploidy, switches per column, flipped haplotypes
    per column, permutation per column).  (The reference's own line order raises IndexError for zero haplotypes before it reaches its
    early return for them; here both early returns are taken.)"""
    assert len(phasing0) == len(phasing1)
    if len(phasing0) == 0 or len(phasing0[0]) == 0:
        return SwitchFlips(), None, None, None
    job = CompareJob(phasing0, phasing1, switch_cost, flip_cost, want_path=True)
    res = switch_flips_batch([job], device=device, host=host)[0]
    result = SwitchFlips(res.switches / job.ploidy, res.flips / job.ploidy)
    return result, res.switches_in_column.tolist(), [np.flatnonzero(row).tolist() for row in res.flipped], res.perms.tolist()


def compute_switch_flips_poly(phasing0, phasing1, switch_cost=1, flip_cost=1, device: int = 0, host: bool = False) -> SwitchFlips:
    """compare.compute_switch_flips_poly: the switches and flips that turn one phasing into the other, each divided by the ploidy."""
    assert len(phasing0) == len(phasing1)
    if len(phasing0) == 0 or len(phasing0[0]) == 0:
        return SwitchFlips()
    job = CompareJob(phasing0, phasing1, switch_cost, flip_cost)
    res = switch_flips_batch([job], device=device, host=host)[0]
    return SwitchFlips(res.switches / job.ploidy, res.flips / job.ploidy)


def compute_switch_errors_poly(phasing0, phasing1, matching_pos=None, device: int = 0, host: bool = False):
    """compare.compute_switch_errors_poly: the switches between the phasings over the positions with matching genotypes, flips priced out
    (flip cost 2 * num_vars * ploidy + 1)."""
    assert len(phasing0) == len(phasing1)
    assert len(phasing0) >= 2
    p0, p1 = phasing_array(phasing0), phasing_array(phasing1)
    assert p0.shape == p1.shape
    n, k = p0.shape
    flip_cost = float(2 * n * k + 1)
    if matching_pos is None:
        job = CompareJob(p0, p1, 1.0, flip_cost, matched_only=True)
    else:
        keep = np.asarray(list(matching_pos), dtype=np.int64)
        job = CompareJob(p0[keep], p1[keep], 1.0, flip_cost)
    res = switch_flips_batch([job], device=device, host=host)[0]
    assert res.flips == 0
    return res.switches / k


def compare_block(phasing0, phasing1, device: int = 0, host: bool = False) -> PhasingErrors:
    """compare.compare_block."""
    assert len(phasing0) == len(phasing1)
    return compare_blocks([(phasing0, phasing1)], device=device, host=host)[0]
