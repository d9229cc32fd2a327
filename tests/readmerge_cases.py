"""Cases of the read merging (whatshap_amd.readmerge): the specs of the recorded cases and the seeded generator of the random ones, the
stand-in read sets both the reference's ``ReadMerger`` and ours are called with, the loader of what the reference recorded
(tests/golden/readmerge_cases.json.gz, written by tests/golden/make_readmerge_golden.py), and the array-level problem of the benchmark.

Inputs are generated, not stored: every number of a recorded case comes from ``random.Random(seed)`` or is spelled out in its spec, and
the golden file keeps the SHA-256 of every generated input, so a drifting generator is noticed before any result is compared.

A case's data is ``dict(reads=[[[position, allele, quality], ...], ...])`` in input order; its spec carries the four constructor
arguments of ``ReadMerger``.  The thresholds the cases are built around: with error_rate 0.15 the base of the logarithm is 17, so
(10^6, 10^3) gives thr_diff 5 and thr_neg_diff 3, (100, 1000) gives 2 and 3, and (10^-6, 10^-3) gives -3 and -1.
"""
import gzip
import hashlib
import json
import os
import random

import numpy as np

from whatshap_amd.core import Read, ReadSet

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "readmerge_cases.json.gz")

DEFAULTS = dict(error_rate=0.15, max_error_rate=0.25, positive_threshold=1000000, negative_threshold=1000)


# ---------------------------------------------------------------------------------------------- stand-in objects
def readset_of(data):
    rs = ReadSet()
    for k, variants in enumerate(data["reads"]):
        read = Read(f"in{k}")
        for position, allele, quality in variants:
            read.add_variant(position, allele, quality)
        rs.add(read)
    return rs


def canonical_reads(readset):
    """A merged read set as plain lists: [[name, [[position, allele, quality], ...]], ...]."""
    return [[read.name, [[int(v.position), int(v.allele), int(v.quality)] for v in read]] for read in readset]


def input_sha256(data):
    return hashlib.sha256(json.dumps(data, sort_keys=True, separators=(",", ":")).encode()).hexdigest()


def merger_args(spec):
    return spec["error_rate"], spec["max_error_rate"], spec["positive_threshold"], spec["negative_threshold"]


# ---------------------------------------------------------------------------------------------- specs
def _spec(name, kind, expect_error=None, **kw):
    spec = dict(DEFAULTS, name=name, kind=kind, expect_error=expect_error)
    spec.update(kw)
    return spec


def _explicit(name, reads, **kw):
    return _spec(name, "explicit", data=dict(reads=[[list(v) for v in read] for read in reads]), **kw)


def _built(name, reads, seed, **kw):
    """reads: [dict(begin, len, hap=0 | 1, flips=[list indices], step=1, quality=None)] -- read k lists the positions begin, begin + step,
    ...; its alleles follow haplotype `hap` of a seeded template (haplotype 1 is the complement) with the listed entries flipped."""
    return _spec(name, "built", seed=seed, reads=reads, **kw)


def _r(begin, length, hap=0, flips=(), step=1, quality=None):
    return dict(begin=begin, len=length, hap=hap, flips=list(flips), step=step, quality=quality)


def _same(alleles, begin=0, quality=10):
    """An explicit read of consecutive positions from `begin` with the alleles of a 0 / 1 string."""
    return [(begin + k, int(c), quality) for k, c in enumerate(alleles)]


def explicit_specs():
    specs = []
    # lengths and shifts: read 0 of every edge length, partners that start 0, 1, 63, 64 and 65 entries into it, of lengths around the
    # word size too -- the overlap ends inside the last word of the one or of the other
    for len_j in (1, 63, 64, 65, 127, 128, 129):
        reads = [_r(0, len_j, flips=[k for k in (0, 62, 63, 64, 126, 127, 128) if k < len_j and k % 3 == 0])]
        for start in (0, 1, 63, 64, 65):
            if start < len_j:
                reads += [_r(start, len_i, hap=(start + len_i) & 1, flips=[f for f in (0, 5, 63, 64) if f < len_i and (f + start) % 2]) for len_i in (1, 63, 64, 65, 130)]
        specs.append(_built(f"shift_len_j_{len_j}", reads, seed=100 + len_j))
    # the same with noisy reads, so that mismatch counts are spread over all words
    specs.append(_spec("shift_noisy", "noisy", seed=77, begins=[0, 0, 1, 1, 63, 63, 64, 64, 65, 65, 127, 128, 129, 130], lengths=[129, 200, 64, 127, 65, 1, 63, 128, 129, 64, 70, 66, 65, 3],
                       p_error=0.12, max_error_rate=0.5, positive_threshold=100))
    # ordering
    specs.append(_built("equal_begins", [_r(10, 20), _r(10, 12, flips=[3]), _r(10, 30, hap=1), _r(10, 9), _r(10, 1), _r(11, 15, hap=1)], seed=3))
    specs.append(_built("no_partner_and_last", [_r(0, 10), _r(2, 10), _r(500, 10), _r(1000, 8), _r(1003, 8), _r(5000, 4)], seed=4))
    # unsorted input, hang < 0: len_j + hang > 0 (start 15 of 20, and 8 of 30) and clamped to 0
    specs.append(_built("unsorted_negative_hang", [_r(50, 20), _r(45, 30), _r(23, 40, flips=[1]), _r(10, 40), _r(60, 12)], seed=5))
    # read 0 leaves the queue at read 1 (far right); read 2 overlaps it in position again but is not compared with it
    specs.append(_built("dropped_then_overlapped", [_r(0, 30), _r(100, 10), _r(5, 30), _r(2, 20), _r(101, 9)], seed=6))
    # exact thresholds.  (100, 1000): thr_diff 2, thr_neg_diff 3 -- L == 3 is an edge, L == 2 is none
    specs.append(_explicit("overlap_at_thr_neg", [_same("000"), _same("000"), _same("0000000", 100), _same("00", 105), _same("00", 200), _same("00", 200)],
                           positive_threshold=100))
    # (10^6, 10^3): thr_diff 5 -- match - mismatch of 5 (5 of 5, 6 of 7) and of 4 (4 of 4, 5 of 6)
    specs.append(_explicit("difference_at_thr", [_same("00000"), _same("00000"), _same("0000000", 100), _same("0001000", 100), _same("0000", 200), _same("0000", 200),
                                                 _same("000000", 300), _same("001000", 300)]))
    # quotients exactly at the bound and just beyond it
    specs.append(_explicit("quotient_quarter", [_same("0000"), _same("0100"), _same("00000000", 100), _same("01000100", 100), _same("0000000", 200), _same("0100100", 200)],
                           positive_threshold=100, max_error_rate=0.25))
    specs.append(_explicit("quotient_tenth", [_same("0" * 10), _same("0" * 9 + "1"), _same("0" * 30, 100), _same("0" * 27 + "111", 100), _same("0" * 19, 200),
                                              _same("0" * 17 + "11", 200), _same("0" * 39, 300), _same("0" * 35 + "1111", 300)], positive_threshold=100, max_error_rate=0.1))
    specs.append(_explicit("quotient_zero_rate", [_same("0" * 12), _same("0" * 12), _same("0" * 12, 100), _same("0" * 11 + "1", 100), _same("1" * 8, 200), _same("0" * 8, 200)],
                           max_error_rate=0.0))
    # merging: a chain whose ends share no edge
    specs.append(_built("chain", [_r(10 * k, 18, flips=[k % 5]) for k in range(7)], seed=8))
    # the input of the merge -> select -> table test: sorted reads of two or more variants each, both haplotypes, some noisy enough to stay alone
    specs.append(_built("phase_input", [_r(2 * k, 9 + (k % 3) * 3, hap=k & 1, flips=[1, 4, 6][:k % 4] if k % 5 == 0 else [k % 7] if k % 3 == 0 else []) for k in range(20)],
                        seed=12))
    specs.append(_built("component_larger_than_a_wave", [_r(k // 8, 12, flips=[k % 12] if k % 3 == 0 else []) for k in range(70)] + [_r(3, 12, hap=1), _r(4, 12, hap=1)], seed=9))
    # a position every member covers, sums that tie (also 0 against 0), qualities of 0
    specs.append(_explicit("ties_and_zero_qualities", [
        [(0, 0, 5), (1, 0, 0), (2, 0, 7), (3, 0, 4), (4, 0, 9), (5, 0, 1), (6, 0, 3), (7, 0, 2)],
        [(0, 1, 5), (1, 1, 0), (2, 0, 7), (3, 0, 4), (4, 0, 9), (5, 0, 1), (6, 0, 3), (7, 0, 2), (9, 0, 0)],
        [(0, 0, 0), (1, 0, 0), (2, 1, 14), (3, 1, 9), (4, 0, 0), (5, 0, 1), (6, 0, 3), (7, 0, 2), (8, 1, 0)],
        [(2, 0, 1), (4, 0, 1), (6, 0, 1), (8, 0, 1), (10, 0, 1), (12, 0, 1)]], max_error_rate=0.3))
    # unsorted input: the representative (smallest id) is not the component's first-begun read; positions come out ascending
    specs.append(_explicit("representative_not_first_begun", [_same("0" * 20, 40, 3), _same("0" * 25, 30, 5), _same("0" * 29 + "1", 22, 7), _same("1" * 8, 200), _same("1" * 12, 195)]))
    # a position listed twice in one read, and negative qualities
    specs.append(_explicit("position_twice_negative_quality", [[(5, 0, 4), (5, 1, 9), (6, 0, -3), (7, 0, 2), (8, 0, 2), (9, 0, 2)],
                                                               [(5, 0, 1), (6, 0, -3), (7, 0, 2), (8, 0, 2), (9, 0, 2), (9, 1, 2)]], positive_threshold=100, max_error_rate=0.5))
    # not-blue edges: thresholds below 1 (thr_diff -3, thr_neg_diff -1).  A - B and B - C are blue only, A - C is blue and not blue: the
    # removal loop takes A - C, then an edge of A - B - C
    low = dict(positive_threshold=1e-6, negative_threshold=1e-3, max_error_rate=0.5)
    a, b, c = _same("0" * 10), _same("0" * 20), _same("11111" + "0" * 15)
    specs.append(_explicit("not_blue_cuts_a_component", [a, b, c], **low))
    # ... and with D the not-blue edge A - D comes when A is cut off already: it lies between two components
    specs.append(_explicit("not_blue_between_components", [a, b, c, _same("11111" + "0" * 15)], **low))
    specs.append(_explicit("not_blue_everywhere", [_same("01" * 6), _same("10" * 6), _same("0011" * 3), _same("1" * 12), _same("0" * 12), _same("0110" * 3, 3)], **low))
    # exceptions, the empty read set, one read alone
    specs.append(_explicit("error_allele_outside", [_same("0000000"), [(0, 0, 5), (1, 2, 5), (2, 0, 5)], []], expect_error="AssertionError"))
    specs.append(_explicit("error_read_without_variants", [_same("0000000"), [], [(0, 3, 5)]], expect_error="IndexError"))
    specs.append(_explicit("empty_readset", []))
    specs.append(_explicit("one_read", [_same("0110100")]))
    return specs


def random_specs():
    """The generator the closed form was checked with: 1 - 25 reads over 40 positions, mixed error rates, both input orders, five
    threshold pairs, three maximum error rates."""
    specs = []
    pairs = [(1000000, 1000), (100, 1000), (10, 10), (1e-6, 1e-3), (0.5, 0.01)]
    for k in range(40):
        specs.append(_spec(f"random_{k}", "random", seed=5000 + k, n_reads=1 + (k * 7) % 25, n_positions=40, p_error=(0.0, 0.05, 0.15, 0.3)[k % 4], sort=bool(k & 1),
                           positive_threshold=pairs[k % 5][0], negative_threshold=pairs[k % 5][1], max_error_rate=(0.25, 0.5, 0.1)[k % 3],
                           error_rate=(0.15, 0.05)[(k // 5) % 2]))
    return specs


def all_specs():
    specs = explicit_specs() + random_specs()
    assert len({s["name"] for s in specs}) == len(specs)
    return specs


def materialize(spec):
    """The complete input of a case as plain data."""
    if spec["kind"] == "explicit":
        return spec["data"]
    rng = random.Random(spec["seed"])
    if spec["kind"] == "built":
        template = [rng.randrange(2) for _ in range(8192)]
        reads = []
        for r in spec["reads"]:
            variants = []
            for t in range(r["len"]):
                position = r["begin"] + t * r["step"]
                allele = template[position % 8192] ^ r["hap"] ^ (1 if t in r["flips"] else 0)
                variants.append([position, allele, r["quality"] if r["quality"] is not None else rng.randint(1, 40)])
            reads.append(variants)
        return dict(reads=reads)
    if spec["kind"] == "noisy":
        template = [rng.randrange(2) for _ in range(1024)]
        reads = []
        for begin, length in zip(spec["begins"], spec["lengths"]):
            hap = rng.randrange(2)
            reads.append([[begin + t, template[begin + t] ^ hap ^ (rng.random() < spec["p_error"]), rng.randint(0, 30)] for t in range(length)])
        return dict(reads=reads)
    assert spec["kind"] == "random"
    n_pos = spec["n_positions"]
    positions = sorted(rng.sample(range(100, 100 + 3 * n_pos), n_pos))
    template = [rng.randrange(2) for _ in range(n_pos)]
    reads = []
    for _ in range(spec["n_reads"]):
        length = rng.randint(1, 20)
        first = rng.randrange(n_pos)
        covered = [x for x in range(first, min(first + length, n_pos)) if x == first or rng.random() < 0.85]
        hap = rng.randrange(2)
        reads.append([[positions[x], template[x] ^ hap ^ (rng.random() < spec["p_error"]), rng.randint(0, 40)] for x in covered])
    if spec["sort"]:
        reads.sort(key=lambda read: read[0][0])
    return dict(reads=reads)


def load_golden():
    with gzip.open(GOLDEN, "rb") as f:
        return json.loads(f.read().decode())


# ---------------------------------------------------------------------------------------------- the benchmark's problem
def bench_reads(n_variants=200000, coverage=20, seed=1, n_reads=None):
    """One chromosome of long reads before the selection, as arrays (read_ptr, position, allele, quality): the read set of the phase
    benchmark's headline (whatshap_amd.synthetic.synthetic_block: 200 000 variants, a read of 40 consecutive variants every 2 variants
    -- coverage 20, about 100 000 reads of 36 entries --, 2 % allele errors, phred 5 .. 40, 10 % of the interior entries dropped) with
    ONE change: a variant's position is its index, not 1000 * (index + 1).  The reference closes a read's window at begin + len, a
    position plus a count: at a spacing of 1000 no window reaches the next read and no pair is compared at all, at a spacing of 1 the
    window is the read's own span -- every read meets the 15 to 20 reads that begin inside it -- which is the most the merging can cost.
    ``n_reads``: only the first reads (the CPU baseline)."""
    from whatshap_amd.synthetic import synthetic_block

    p = synthetic_block(n_variants, coverage, seed)
    read_ptr = p.read_ptr
    if n_reads is not None and n_reads < read_ptr.size - 1:
        read_ptr = read_ptr[:n_reads + 1].copy()
    n_entries = int(read_ptr[-1])
    position = (p.var_position[:n_entries].astype(np.int64) // 1000) - 1
    return read_ptr, position, p.var_allele[:n_entries].copy(), p.var_quality[:n_entries].astype(np.int64)
