"""``GenotypeDPTable`` -- the drop-in for ``whatshap.core.GenotypeDPTable`` (``whatshap/core.pyx:581-602``; its caller is
``whatshap/cli/genotype.py:357-368``), SURVEY.md section 8 row (f3): the forward-backward genotyper over the same columns,
indexing scheme and pedigree partitions as the phasing table (``src/genotypedptable.cpp``).

The whole computation runs on the device behind the C ABI (``whamd_genotype_likelihoods``,
``whatshap_amd/csrc/genotype_device.hip``); there is no CPU fallback.  The reference computes in ``long double``, the
device in f64: likelihoods agree to a relative tolerance (tests: 1e-9), not bit for bit.

The table's priors -- ``compute_genotypes`` (``core.pyx:603``, called at ``cli/genotype.py:243``) and the regularisation loop behind it --
are the second half of this module: ``compute_genotypes``, ``prior_likelihoods``, ``prior_genotypes_batch``, ``determine_genotype``.
Those are held to the reference bit for bit.
"""
import ctypes as C
from typing import Iterable, List, Optional, Sequence

import numpy as np

from . import _native, core


class GenotypeDPTable:
    """``GenotypeDPTable(numeric_sample_ids, readset, recombcost, pedigree, positions=None)`` -- same constructor as the
    reference; like there, the constructor does all the work.  ``pedigree`` must carry genotype likelihoods (the priors)
    for every individual and variant (the reference asserts that, ``src/transitionprobabilitycomputer.cpp:66``)."""

    def __init__(self, numeric_sample_ids, readset, recombcost, pedigree, positions: Optional[Iterable[int]] = None,
                 device: int = 0, window: int = 0, problem: Optional[_native.ProblemArrays] = None):
        self.numeric_sample_ids = numeric_sample_ids
        self.pedigree = pedigree
        if problem is None:
            problem = self._problem(readset, recombcost, pedigree, positions)
        self._problem_arrays = problem
        if problem.positions is not None:
            n_columns = int(problem.positions.size)
        else:
            n_columns = int(np.unique(problem.var_position).size)
        self._individual_ids = [int(x) for x in problem.individual_id]
        self._gl, self._stats = _native.genotype_likelihoods(problem, n_columns, device=device, window=window)

    @staticmethod
    def _problem(readset, recombcost, pedigree, positions):
        if isinstance(pedigree, core.Pedigree):
            return core.problem_from_objects(readset, recombcost, pedigree, False, positions)
        from . import ingest

        compiled = ingest.load()
        if compiled is None:
            raise TypeError("a reference Pedigree needs the compiled ingestion (whatshap_amd.ingest) or whatshap_amd.core.Pedigree")
        return core.problem_from_reference_objects(compiled, readset, recombcost, pedigree, False, positions)

    def get_genotype_likelihoods(self, sample_id, pos: int) -> core.PhredGenotypeLikelihoods:
        numeric = self.numeric_sample_ids[sample_id]
        index = None
        for i in range(len(self._individual_ids) - 1, -1, -1):   # Pedigree::id_to_index: the last individual with that id
            if self._individual_ids[i] == numeric:
                index = i
                break
        if index is None:
            raise RuntimeError(f"Individual with ID {numeric} not present in pedigree.")
        return core.PhredGenotypeLikelihoods([float(x) for x in self._gl[index, pos]])

    def get_stats(self) -> dict:
        return dict(self._stats)


# ---------------------------------------------------------------------------------------------- the priors: compute_genotypes
# The first compute step of `whatshap genotype` (src/genotyper.cpp through core.pyx:603, called at cli/genotype.py:243) and the loop that
# regularises its output (cli/genotype.py:245-262).  The native library validates and maps entry positions to columns on the host, and
# transposes the reads, orders every column's run by entry index and walks the chains on the device (csrc/priorgt_device.hip);
# ``host=True`` walks them on one host thread of the debug library instead (test infrastructure).  Results equal the reference's bit for
# bit.  There is no CPU fallback: without a device the native call raises.
class PriorProblem:
    """One sample on one chromosome, as arrays: the reads as a CSR of (position, allele, quality) and the position list (``None``: the
    sorted positions of the entries, as ``ReadSet.get_positions``).  ``constant`` and ``gt_prob`` are those of the regularisation, applied
    only with ``want_regularized``."""

    def __init__(self, read_ptr, entry_position, entry_allele, entry_quality, positions=None, constant: float = 0.0, gt_prob: float = 0.0,
                 want_regularized: bool = False):
        self.read_ptr = np.ascontiguousarray(read_ptr, dtype=np.uint64)
        if self.read_ptr.size == 0:
            self.read_ptr = np.zeros(1, dtype=np.uint64)
        self.n_reads = self.read_ptr.size - 1
        self.entry_position = self._as_uint32(entry_position, "an entry position")
        if isinstance(entry_allele, np.ndarray) and entry_allele.dtype == np.uint8:
            self.entry_allele = np.ascontiguousarray(entry_allele)   # (the library passes over everything above 1)
        else:
            allele = np.asarray(entry_allele, dtype=np.int64)
            self.entry_allele = np.ascontiguousarray(np.where((allele == 0) | (allele == 1), allele, 255), dtype=np.uint8)
        if isinstance(entry_quality, np.ndarray) and entry_quality.dtype == np.uint32:
            self.entry_quality = np.ascontiguousarray(entry_quality)
        else:
            quality = np.asarray(entry_quality, dtype=np.int64)
            if quality.size and quality.min() < 0:
                raise ValueError("a negative quality (the reference's phred scores are unsigned)")
            self.entry_quality = np.ascontiguousarray(np.minimum(quality, (1 << 32) - 1), dtype=np.uint32)
        n_entries = int(self.read_ptr[-1])
        if not (self.entry_position.size == self.entry_allele.size == self.entry_quality.size == n_entries):
            raise ValueError("entry arrays and read_ptr disagree (mismatched lengths)")
        if positions is None:
            self.positions = np.unique(self.entry_position)
        else:
            self.positions = self._as_uint32(positions if isinstance(positions, np.ndarray) else list(positions), "a position")
        self.constant = float(constant)
        self.gt_prob = float(gt_prob)
        self.want_regularized = bool(want_regularized)

    @staticmethod
    def _as_uint32(values, what):
        if isinstance(values, np.ndarray) and values.dtype == np.uint32:
            return np.ascontiguousarray(values)   # (arrays of the library's own type are taken as they are: no copy)
        wide = np.asarray(values, dtype=np.int64)
        if wide.size and (wide.min() < 0 or wide.max() >= 1 << 32):
            raise ValueError(what + " outside uint32")
        return np.ascontiguousarray(wide, dtype=np.uint32)

    @classmethod
    def from_readset(cls, readset, positions=None, **kwargs) -> "PriorProblem":
        """From a ``whatshap_amd.core.ReadSet``, or -- through the compiled ingestion -- the reference's ``ReadSet``; any other iterable
        of reads is walked through its public interface."""
        read_ptr = pos = alle = qual = None
        if not isinstance(readset, core.ReadSet):
            from . import ingest

            compiled = ingest.load()
            if compiled is not None:
                try:
                    read_ptr, pos, alle, qual, _samples = compiled.flatten_readset(readset)
                except TypeError:
                    pass
        if read_ptr is None:
            read_ptr, pos, alle, qual, _samples = core._flatten_readset(readset)
        return cls(read_ptr, pos, alle, qual, positions, **kwargs)

    def view(self) -> _native.PriorGenotypesView:
        P = _native._ptr
        return _native.PriorGenotypesView(self.positions.size, P(self.positions, C.c_uint32), self.n_reads, P(self.read_ptr, C.c_uint64),
                                          P(self.entry_position, C.c_uint32), P(self.entry_allele, C.c_uint8), P(self.entry_quality, C.c_uint32),
                                          self.constant, self.gt_prob, 1 if self.want_regularized else 0, 0)


class PriorResult:
    """Per position ``gl`` [n, 3] and ``genotype`` (0 .. 2, -1: none); with ``want_regularized`` ``reg`` [n, 3] and ``reg_genotype``
    (without: zeros and -1); ``stats``."""

    def __init__(self, gl, genotype, reg, reg_genotype, stats):
        self.gl, self.genotype, self.reg, self.reg_genotype, self.stats = gl, genotype, reg, reg_genotype, stats


def prior_genotypes_batch(problems: Sequence[PriorProblem], device: int = 0, host: bool = False, stats: Optional[list] = None) -> List[PriorResult]:
    """Every problem (sample x chromosome) in one native call: one upload, ``_native.PRIOR_GENOTYPES_LAUNCHES`` launches whatever the
    problems (none when no entry counts), one download.  ``stats``, if given, receives one dict per problem (its counts; launches and
    times are those of the whole call)."""
    P = _native._ptr
    with _native.batch_handle(host, [p.view() for p in problems], "whamd_prior_genotypes", "whamd_debug_prior_genotypes_host",
                              "whamd_prior_genotypes_destroy", device=device) as (L, h):
        out = []
        for k in range(len(problems)):
            cnt = L.whamd_prior_genotypes_count(h, k)
            gl, reg = np.zeros((cnt, 3), dtype=np.float64), np.zeros((cnt, 3), dtype=np.float64)
            gt, reg_gt = np.zeros(cnt, dtype=np.int8), np.zeros(cnt, dtype=np.int8)
            _native.checked(L, L.whamd_prior_genotypes_get(h, k, P(gl, C.c_double), P(gt, C.c_int8), P(reg, C.c_double), P(reg_gt, C.c_int8)))
            ts = _native.read_stats(L, "whamd_prior_genotypes_get_stats", _native.PriorGenotypesStats, h, k)
            out.append(PriorResult(gl, gt, reg, reg_gt, ts))
            if stats is not None:
                stats.append(dict(ts))
        return out


def int_to_diploid_biallelic_gt(numeric_repr: int) -> core.Genotype:
    """cli/genotype.py:41-52: 0, 1, 2 -> 0/0, 0/1, 1/1; anything else the empty genotype."""
    if numeric_repr == 0:
        return core.Genotype([0, 0])
    if numeric_repr == 1:
        return core.Genotype([0, 1])
    if numeric_repr == 2:
        return core.Genotype([1, 1])
    return core.Genotype([])


def compute_genotypes(readset, positions=None, device: int = 0, host: bool = False, stats: Optional[list] = None):
    """``whatshap.core.compute_genotypes`` (core.pyx:603): ``(genotypes, genotype_likelihoods)`` -- per position a ``Genotype`` (empty
    where the error probability is 0.1 or more) and a 3-tuple of floats, the reference's values bit for bit.  Raises ``ValueError``
    (naming the read) where the reference throws or asserts: unsorted reads, a read with unsorted positions, a read whose first or last
    position is not in ``positions``."""
    problem = PriorProblem.from_readset(readset, positions)
    res = prior_genotypes_batch([problem], device=device, host=host, stats=stats)[0]
    return [int_to_diploid_biallelic_gt(g) for g in res.genotype.tolist()], [tuple(row) for row in res.gl.tolist()]


def prior_likelihoods(readset, positions, constant: float, gt_qual_threshold: float, device: int = 0, host: bool = False, stats: Optional[list] = None):
    """compute_genotypes and the loop of cli/genotype.py:245-262 in one call: ``(genotypes, regularized)`` -- per position the genotype
    ``determine_genotype`` gives the regularised likelihoods at ``gt_prob = 1 - 10 ** (-gt_qual_threshold / 10)``, and those likelihoods
    as ``PhredGenotypeLikelihoods``; what ``run_genotype`` hands to ``set_genotypes_of`` and ``set_genotype_likelihoods_of``."""
    gt_prob = 1.0 - (10 ** (-gt_qual_threshold / 10.0))
    problem = PriorProblem.from_readset(readset, positions, constant=constant, gt_prob=gt_prob, want_regularized=True)
    res = prior_genotypes_batch([problem], device=device, host=host, stats=stats)[0]
    return ([int_to_diploid_biallelic_gt(g) for g in res.reg_genotype.tolist()], [core.PhredGenotypeLikelihoods(row) for row in res.reg.tolist()])


def determine_genotype(likelihoods, threshold_prob: float) -> core.Genotype:
    """cli/genotype.py:55-69, on the host (for the table's results): the likeliest genotype if it is alone at the top and above the
    threshold, else the empty one.  ``likelihoods``: ``PhredGenotypeLikelihoods`` (ours or the reference's) or three floats."""
    values = list(likelihoods)   # (both likelihood classes iterate in genotype-index order)
    to_sort = [(values[0], 0), (values[1], 1), (values[2], 2)]
    to_sort.sort(key=lambda x: x[0])
    if to_sort[2][0] > to_sort[1][0] and to_sort[2][0] > threshold_prob:
        return int_to_diploid_biallelic_gt(to_sort[2][1])
    return int_to_diploid_biallelic_gt(-1)
