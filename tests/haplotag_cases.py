"""Cases of haplotagging (whatshap_amd.haplotag): the seeded generators of their inputs, the stand-in objects both the reference's
function and ours are called with, the loader of what the reference recorded (tests/golden/haplotag_cases.json.gz, written by
tests/golden/make_haplotag_golden.py), and the array-level problems of the device tests and of the benchmark.

Inputs are generated, not stored: every number of a recorded case comes from ``random.Random(seed)`` or is spelled out in its spec, and
the golden file keeps the SHA-256 of every generated input, so a drifting generator is noticed before any result is compared.
"""
import gzip
import hashlib
import json
import os
import random

import numpy as np

from whatshap_amd.core import Read

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "haplotag_cases.json.gz")
CHROMOSOME = "chr1"


# ---------------------------------------------------------------------------------------------- stand-in objects
class _Variant:
    def __init__(self, position):
        self.position = position


class _Genotype:
    def __init__(self, hom):
        self._hom = hom

    def is_homozygous(self):
        return self._hom


class _Phase:
    def __init__(self, block_id, phase):
        self.block_id, self.phase = block_id, phase


class CaseTable:
    """What prepare_haplotag_information reads of a VariantTable."""

    def __init__(self, data):
        self.chromosome = data["chromosome"]
        self.variants = [_Variant(p) for p in data["positions"]]
        self._samples = data["samples"]

    def genotypes_of(self, sample):
        return [_Genotype(bool(h)) for h in self._samples[sample]["hom"]]

    def phases_of(self, sample):
        return [None if ph is None else _Phase(ph[0], tuple(ph[1])) for ph in self._samples[sample]["phases"]]


class CaseReader:
    """What it reads of a PhasedInputReader: read() returns (read set, None); the read set is a list of whatshap_amd.core.Read."""

    def __init__(self, data):
        self._samples = data["samples"]
        self.calls = []

    def read(self, chromosome, variants, sample, regions=None):
        self.calls.append((chromosome, [v.position for v in variants], sample, regions))
        reads = []
        for r in self._samples[sample]["reads"]:
            read = Read(r["name"], 0, 0, 0, r["start"], r["bx"], -1, -1, r["chromosome"], r["sub"], r["supp"], r["end"], r["rev"])
            for pos, allele, quality in r["variants"]:
                read.add_variant(pos, allele, quality)
            reads.append(read)
        return reads, None


def call_args(spec, data):
    """The positional arguments of prepare_haplotag_information for a case."""
    return (CaseTable(data), list(data["sample_order"]), CaseReader(data), None, spec["ignore_linked_read"], spec["cutoff"], spec["ploidy"])


def canonical(results):
    """The four results of prepare_haplotag_information as plain sorted lists (the keys by their four / three fields)."""
    bx, reads, n_multiple, primary = results
    return dict(
        reads=sorted([k.read_name, k.chromosome, bool(k.is_supplementary), k.sub_alignment_id, int(v[0]), int(v[1]), int(v[2])] for k, v in reads.items()),
        bx={str(tag): [[int(a), int(b), int(c)] for a, b, c in lst] for tag, lst in sorted(bx.items()) if lst},
        n_multiple_phase_sets=int(n_multiple),
        primary=sorted([k.read_name, k.chromosome, bool(k.is_supplementary), k.sub_alignment_id, int(v.reference_start), int(v.reference_end), bool(v.is_reverse)]
                       for k, v in primary.items()))


def input_sha256(data):
    return hashlib.sha256(json.dumps(data, sort_keys=True, separators=(",", ":")).encode()).hexdigest()


# ---------------------------------------------------------------------------------------------- specs
def _read(name, variants, start=0, bx="", sub="____1", supp=False, end=None, rev=False, chromosome=CHROMOSOME):
    return dict(name=name, variants=[list(v) for v in variants], start=start, bx=bx, sub=sub, supp=supp, end=start + 100 if end is None else end, rev=rev,
                chromosome=chromosome)


def _explicit(name, ploidy, table, reads, ignore_linked_read=True, cutoff=50000, expect_error=None, more_samples=None):
    """table: [(position, block_id or None, phase tuple)]; reads: list of _read()."""
    samples = {"s0": dict(phases=[None if b is None else [b, list(ph)] for _, b, ph in table], hom=[0] * len(table), reads=reads)}
    order = ["s0"]
    for sname, (stable, sreads) in (more_samples or {}).items():
        assert [p for p, _, _ in stable] == [p for p, _, _ in table]
        samples[sname] = dict(phases=[None if b is None else [b, list(ph)] for _, b, ph in stable], hom=[0] * len(stable), reads=sreads)
        order.append(sname)
    return dict(name=name, kind="explicit", ploidy=ploidy, ignore_linked_read=ignore_linked_read, cutoff=cutoff, expect_error=expect_error,
                data=dict(chromosome=CHROMOSOME, positions=[p for p, _, _ in table], sample_order=order, samples=samples))


def explicit_specs():
    specs = []
    A, B, C3 = 100, 200, 300   # block ids
    two = [(10, A, (0, 1)), (20, B, (0, 1)), (30, A, (1, 0)), (40, B, (1, 0)), (50, A, (0, 1)), (60, B, (0, 1))]   # two interleaved phase sets
    # single-read ties between two phase sets, both orders of first encounter; a strict winner that comes second
    specs.append(_explicit("tie_phasesets_a_first", 2, two, [_read("r1", [(10, 0, 7), (20, 0, 7)]), _read("r2", [(10, 0, 7), (20, 0, 4), (40, 1, 3)])]))
    specs.append(_explicit("tie_phasesets_b_first", 2, two, [_read("r1", [(20, 1, 9), (30, 0, 9)]), _read("r2", [(20, 0, 5), (30, 1, 2), (50, 0, 3)]),
                                                               _read("r3", [(10, 0, 3), (20, 0, 8)])]))
    # best and second-best haplotype equal: quality 0, unassigned, still counted in n_multiple_phase_sets (r1); without a second phase set not counted (r2)
    specs.append(_explicit("quality_zero", 2, two, [_read("r1", [(10, 0, 5), (30, 0, 5), (20, 0, 2), (40, 0, 2)]), _read("r2", [(10, 0, 4), (50, 1, 4)]),
                                                     _read("r3", [(10, 0, 4), (50, 1, 5)])]))
    three = [(10, A, (0, 1, 1)), (20, A, (1, 0, 1)), (30, A, (1, 1, 0)), (40, B, (0, 0, 1)), (50, B, (1, 0, 0))]
    specs.append(_explicit("three_equal_haplotypes", 3, three, [_read("r1", [(10, 1, 6), (20, 1, 6), (30, 1, 6)]),        # 12 12 12
                                                                 _read("r2", [(10, 1, 6), (20, 1, 6), (30, 1, 5)]),        # 11 11 12 -> hap 2, quality 1
                                                                 _read("r3", [(10, 0, 6), (20, 0, 6), (40, 1, 1)]),        # A: 6 6 0 (quality 0), B: 0 0 1
                                                                 _read("r4", [(40, 0, 3), (50, 0, 3), (10, 0, 6)])]))      # B: 3 6 3, A: 6 0 0 -> tie on 6, B first
    # phasing alleles outside {0, 1}: they match nothing, and a phase set nothing matched does not exist
    odd = [(10, A, (2, 1)), (20, A, (-1, 0)), (30, B, (2, 2)), (40, B, (0, 7)), (50, C3, (1, 1)), (60, C3, (0, 0)), (70, None, (0, 1))]
    specs.append(_explicit("phasing_outside_01", 2, odd, [_read("r1", [(10, 1, 5), (20, 1, 3)]), _read("r2", [(10, 0, 5), (30, 0, 4), (30, 1, 4)]),
                                                           _read("r3", [(30, 1, 9)]), _read("r4", [(30, 0, 2), (40, 0, 6), (10, 1, 6)]),
                                                           _read("r5", [(50, 0, 3), (60, 1, 3)]), _read("r6", [(50, 1, 3), (60, 1, 3), (20, 0, 1)]),
                                                           _read("r7", [(40, 0, 1), (50, 1, 8)])]))
    # negative and large qualities: sums beyond 2^31, a maximum that belongs to a haplotype nothing matched
    big = (1 << 31) - 1
    specs.append(_explicit("extreme_qualities", 2, two, [_read("r1", [(10, 0, big), (30, 1, big), (50, 0, big), (20, 0, 5)]),
                                                          _read("r2", [(10, 0, -5)]), _read("r3", [(10, 0, -(1 << 31)), (30, 1, -(1 << 31)), (20, 1, -7)]),
                                                          _read("r4", [(10, 0, big), (30, 0, big), (50, 0, big), (50, 1, big), (20, 1, big)]),
                                                          _read("r5", [(10, 0, -3), (30, 0, -3)])]))
    # reads with 0, 1, 2 variants
    specs.append(_explicit("short_reads", 2, two, [_read("r0", []), _read("r1", [(10, 1, 30)]), _read("r2", [(10, 1, 30), (30, 0, 11)]), _read("r3", []),
                                                    _read("r4", [(20, 0, 1), (10, 1, 1)])]))
    # linked reads: cutoff exactly met (r2) and exceeded by one (r3); r4 reachable from the seeds r1 and r3, the earlier takes it when in reach
    linked = [_read("r1", [(10, 0, 9)], start=1000, bx="T1"), _read("r2", [(30, 1, 4)], start=1500, bx="T1"), _read("r3", [(50, 1, 20)], start=1501, bx="T1"),
              _read("r4", [(10, 0, 2), (20, 0, 30)], start=1400, bx="T1"), _read("r5", [(20, 1, 3)], start=1000, bx="T2"), _read("r6", [(10, 1, 6)], start=1100)]
    specs.append(_explicit("linked_cutoff", 2, two, linked, ignore_linked_read=False, cutoff=500))
    specs.append(_explicit("linked_cutoff_ignored", 2, two, linked, ignore_linked_read=True, cutoff=500))
    specs.append(_explicit("linked_cutoff_399", 2, two, linked, ignore_linked_read=False, cutoff=399))
    specs.append(_explicit("linked_cutoff_zero", 2, two, linked, ignore_linked_read=False, cutoff=0))
    # a group dropped at quality 0 (r1 + r2 cancel): its members must not seed again; r3 of another tag does
    dropped = [_read("r1", [(10, 0, 5)], start=100, bx="T1"), _read("r2", [(10, 1, 5)], start=120, bx="T1"), _read("r3", [(10, 1, 5)], start=130, bx="T2"),
               _read("r4", [(30, 1, 8)], start=90000, bx="T1")]
    specs.append(_explicit("linked_group_dropped", 2, two, dropped, ignore_linked_read=False, cutoff=1000))
    # representations: a name that ends in its sub-alignment id loses it; two reads with one representation (the second is skipped);
    # supplementary and primary of one name are two representations
    sub = [_read("q1____1", [(10, 0, 5)], sub="____1"), _read("q1____2", [(10, 1, 6)], sub="____2", supp=True), _read("q1", [(30, 0, 9), (20, 0, 3)], sub="____2", supp=True),
           _read("q2", [(10, 1, 4)], sub="____1"), _read("q2____1", [(10, 0, 40)], sub="____1"), _read("q3____1", [(20, 1, 4)], sub="____1", supp=True, rev=True),
           _read("q4ab", [(10, 0, 3)], sub="ab"), _read("q5", [(10, 0, 3)], sub="____7", start=77, end=99, rev=True),
           _read("q6", [(10, 1, 2)], sub=""), _read("q7", [(10, 0, 8)], sub="")]   # an empty id: name[:-0] is the empty name, for both
    specs.append(_explicit("representations", 2, two, sub))
    specs.append(_explicit("representations_linked", 2, two, [dict(r, bx="T") for r in sub], ignore_linked_read=False, cutoff=10))
    # two samples sharing read names: the later sample overwrites
    two_b = [(p, b + 1, ph[::-1]) for p, b, ph in two]
    specs.append(_explicit("two_samples", 2, two, [_read("r1____1", [(10, 0, 7)], sub="____1", bx="T"), _read("r2____1", [(20, 0, 3)], sub="____1", bx="T")],
                           ignore_linked_read=False, more_samples={"s1": (two_b, [_read("r1____1", [(10, 0, 9), (30, 1, 1)], sub="____1", bx="T", start=5),
                                                                                  _read("r3____1", [(10, 0, 9), (10, 1, 9)], sub="____1")])}))
    # errors
    specs.append(_explicit("error_ploidy_1", 1, [(10, A, (0,)), (20, A, (1,))], [_read("r1", [(10, 0, 5), (20, 1, 5)])], expect_error="ValueError"))
    p17 = tuple(i & 1 for i in range(17))
    specs.append(_explicit("error_ploidy_17", 17, [(10, A, p17), (20, A, p17[::-1])], [_read("r1", [(10, 0, 5), (20, 1, 6)])], expect_error="ValueError"))
    specs.append(_explicit("error_unknown_position", 2, two, [_read("r1", [(10, 0, 5)]), _read("r2", [(10, 0, 5), (15, 1, 5)])], expect_error="ValueError"))
    specs.append(_explicit("error_unphased_position", 2, odd, [_read("r1", [(70, 0, 5)])], expect_error="ValueError"))
    specs.append(_explicit("error_allele_2", 2, two, [_read("r1", [(10, 0, 5)]), _read("r2", [(10, 2, 5)])], expect_error="ValueError"))
    specs.append(_explicit("error_allele_negative", 2, two, [_read("r1", [(10, -1, 5)])], expect_error="ValueError"))
    return specs


def random_specs():
    specs = []

    def add(name, ploidy, **kw):
        base = dict(name=name, kind="random", ploidy=ploidy, seed=1000 + len(specs), ignore_linked_read=True, cutoff=50000, expect_error=None, n_variants=60,
                    n_phasesets=3, interleaved=True, n_reads=60, lengths=[0, 1, 2, 3, 5, 8, 13], quality=[1, 60], p_bx=0.0, n_bx=1, p_odd_phase=0.0, p_unphased=0.05,
                    p_supp=0.1, n_samples=1, p_error=0.15, spread=4000)
        assert set(kw) <= set(base)
        base.update(kw)
        specs.append(base)

    for ploidy in (2, 3, 4, 6, 8, 16):
        add(f"mixed_p{ploidy}", ploidy)
        add(f"tie_heavy_p{ploidy}", ploidy, quality=[1, 2], lengths=[1, 2, 2, 3, 4, 6], n_phasesets=4, n_reads=80)
    for n_ps in range(1, 8):
        add(f"phasesets_{n_ps}", 2, n_phasesets=n_ps, lengths=[n_ps, 2 * n_ps, 3 * n_ps + 1, 40], n_variants=80, quality=[1, 9])
    add("consecutive_phasesets", 2, interleaved=False, n_phasesets=5, lengths=[2, 6, 30])
    add("odd_phasings_p4", 4, p_odd_phase=0.3, quality=[1, 5])
    add("negative_qualities", 2, quality=[-20, 20])
    add("huge_qualities", 3, quality=[(1 << 31) - 40, (1 << 31) - 1], lengths=[3, 9, 27])
    add("long_reads", 2, lengths=[70, 130, 300], n_variants=400, n_reads=12, n_phasesets=6)
    add("linked_short_reads", 2, ignore_linked_read=False, p_bx=0.9, n_bx=12, lengths=[0, 1, 1, 2, 3], cutoff=3000, n_reads=150, quality=[1, 1000000])
    add("linked_short_reads_ignored", 2, ignore_linked_read=True, p_bx=0.9, n_bx=12, lengths=[0, 1, 1, 2, 3], cutoff=3000, n_reads=150)
    add("linked_p4", 4, ignore_linked_read=False, p_bx=0.7, n_bx=6, lengths=[1, 2, 4], cutoff=800, n_reads=100, quality=[1, 1000000])
    add("linked_two_samples", 2, ignore_linked_read=False, p_bx=0.8, n_bx=5, cutoff=2000, n_samples=2, n_reads=50, quality=[1, 1000000])
    add("three_samples", 3, n_samples=3, n_reads=40)
    return specs


def all_specs():
    specs = explicit_specs() + random_specs()
    assert len({s["name"] for s in specs}) == len(specs)
    return specs


def materialize(spec):
    """The complete input of a case as plain data (what CaseTable / CaseReader are built from)."""
    if spec["kind"] == "explicit":
        return spec["data"]
    rng = random.Random(spec["seed"])
    ploidy, n_var = spec["ploidy"], spec["n_variants"]
    positions = sorted(rng.sample(range(1000, 1000 + n_var * 100), n_var))
    samples, order = {}, [f"s{k}" for k in range(spec["n_samples"])]
    for sname in order:
        n_ps = spec["n_phasesets"]
        if spec["interleaved"]:   # nested / interleaved phase sets: each variant picks among the sets around its place
            ps_of = [min(n_ps - 1, max(0, (i * n_ps) // n_var + rng.choice((-1, 0, 0, 1)))) for i in range(n_var)]
        else:
            ps_of = [(i * n_ps) // n_var for i in range(n_var)]
        block = [rng.randrange(1, 1 << 40) for _ in range(n_ps)]
        phases, hom = [], []
        for i in range(n_var):
            if rng.random() < spec["p_unphased"]:
                phases.append(None)
            else:
                ph = [rng.randrange(2) for _ in range(ploidy)]
                for h in range(ploidy):
                    if rng.random() < spec["p_odd_phase"]:
                        ph[h] = rng.choice((2, -1, 3))
                phases.append([block[ps_of[i]], ph])
            hom.append(int(rng.random() < 0.1))
        phased = [i for i in range(n_var) if phases[i] is not None]
        reads = []
        for k in range(spec["n_reads"]):
            length = min(rng.choice(spec["lengths"]), len(phased))
            at = rng.randrange(len(phased) - length + 1)
            picked = phased[at:at + length]
            hap = rng.randrange(ploidy)
            variants = []
            for i in picked:
                truth = phases[i][1][hap]
                allele = truth if truth in (0, 1) and rng.random() >= spec["p_error"] else rng.randrange(2)
                variants.append([positions[i], allele, rng.randint(*spec["quality"])])
            start = (positions[picked[0]] if picked else rng.randrange(1000, 1000 + n_var * 100)) - rng.randrange(spec["spread"])
            supp = rng.random() < spec["p_supp"]
            sub = "____%d" % (rng.randrange(2, 4) if supp else 1)
            name = "read%d" % (k if rng.random() < 0.8 else rng.randrange(spec["n_reads"]))   # some names repeat (one representation, or primary + supplementary)
            bx = "BX%d" % rng.randrange(spec["n_bx"]) if rng.random() < spec["p_bx"] else ""
            reads.append(_read(name + sub, variants, start=start, bx=bx, sub=sub, supp=supp, end=start + rng.randrange(100, 20000), rev=rng.random() < 0.5))
        samples[sname] = dict(phases=phases, hom=hom, reads=reads)
    return dict(chromosome=CHROMOSOME, positions=positions, sample_order=order, samples=samples)


def load_golden():
    with gzip.open(GOLDEN, "rb") as f:
        return json.loads(f.read().decode())


# ---------------------------------------------------------------------------------------------- array-level problems (device tests, benchmark)
def array_problem(ploidy, lengths, seed, n_phasesets=3, n_variants=None, quality=(1, 60), window=64, linked=None):
    """A whatshap_amd.haplotag.HaplotagProblem with one read per entry of ``lengths`` (numpy generator ``seed``): every read lists consecutive
    variants from a random place, alleles follow one haplotype with 15 % errors.  Phase sets interleave (variant i belongs to set
    i mod n_phasesets within windows of ``window`` variants, so a read of L variants inside one window meets at most min(L, n_phasesets)).  ``linked`` = (tags,
    cutoff): every read gets one of ``tags`` BX tags."""
    from whatshap_amd.haplotag import HaplotagProblem

    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    n_var = int(n_variants or max(1000, int(lengths.max(initial=1)) + 10))
    positions = np.arange(n_var, dtype=np.int64) * 97 + 1000
    phaseset = (np.arange(n_var) // window) * 1000 + (np.arange(n_var) % n_phasesets)
    phasing = rng.integers(0, 2, size=(n_var, ploidy), dtype=np.int8)
    read_ptr = np.zeros(lengths.size + 1, dtype=np.uint64)
    np.cumsum(lengths, out=read_ptr[1:])
    n_entries = int(read_ptr[-1])
    first = rng.integers(0, np.maximum(n_var - lengths, 0) + 1)
    read_of = np.repeat(np.arange(lengths.size), lengths)
    var = first[read_of] + (np.arange(n_entries) - read_ptr[:-1].astype(np.int64)[read_of])
    hap = rng.integers(0, ploidy, size=lengths.size)
    allele = phasing[var, hap[read_of]].astype(np.int8)
    flip = rng.random(n_entries) < 0.15
    allele[flip] ^= 1
    qual = rng.integers(quality[0], quality[1] + 1, size=n_entries, dtype=np.int64)
    start = positions[np.minimum(first, n_var - 1)] - rng.integers(0, 50, size=lengths.size)
    bx = None
    cutoff = 50000
    if linked is not None:
        bx = rng.integers(0, max(1, min(linked[0], lengths.size)), size=lengths.size).astype(np.uint32)   # (dense ids: below the number of reads)
        cutoff = linked[1]
    return HaplotagProblem(ploidy, positions, phaseset, phasing, read_ptr, positions[var], allele, qual, start, np.arange(lengths.size, dtype=np.uint32), bx,
                           linked is not None, cutoff)


def heavy_tail_lengths(n_reads, seed, mean=30, tail=0.0005, tail_max=60000):
    """Mixed read lengths: geometric around ``mean`` with zeros and ones, and a heavy tail of a few very long reads."""
    rng = np.random.default_rng(seed)
    lengths = rng.geometric(1.0 / mean, size=n_reads) - 1
    long_ones = rng.random(n_reads) < tail
    lengths[long_ones] = rng.integers(100, tail_max, size=int(long_ones.sum()))
    return lengths


def bench_problem(kind, n_reads=2_000_000, seed=7):
    """The problems of scripts/gpu_haplotag_bench.py: "long2" / "long4": n_reads long reads of 30 variants on average (6e7 entries at the
    default size) at ploidy 2 / 4; "linked": short linked reads (0 .. 3 variants, 20 reads per tag on average)."""
    if kind == "linked":
        rng = np.random.default_rng(seed)
        return array_problem(2, rng.integers(0, 4, size=n_reads), seed, n_phasesets=2, n_variants=200_000, window=20_000, linked=(max(1, n_reads // 20), 50000))
    # two interleaved phase sets per window of 20 000 variants: a read meets two, or four where it crosses into the next window
    return array_problem({"long2": 2, "long4": 4}[kind], heavy_tail_lengths(n_reads, seed, tail=0.0002, tail_max=20000), seed, n_phasesets=2, n_variants=200_000,
                         window=20_000)
