"""Cases of haplotagphase (whatshap_amd.haplotagphase): the specs of the recorded cases and the seeded generator of the random ones, the
stand-in objects both the reference's functions and ours are called with, the loader of what the reference recorded
(tests/golden/haplotagphase_cases.json.gz, written by tests/golden/make_haplotagphase_golden.py), and the array-level problems of the
device tests and of the benchmark.

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

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "haplotagphase_cases.json.gz")


# ---------------------------------------------------------------------------------------------- stand-in objects
class _Change:
    """What consensus reads of a VcfVariant."""

    def __init__(self, snv):
        self._snv = snv

    def is_snv(self):
        return self._snv


def call_args(data):
    """What run_haplotagphase builds for one sample (haplotagphase.py:150-167) from a case's data, and the reads."""
    is_homozygous, phased, change, allele_to_id, id_to_allele = {}, {}, {}, {}, {}
    for pos, genotype, is_phased, snv in data["variants"]:
        allele_to_id.setdefault(pos, {})
        id_to_allele.setdefault(pos, {})
        for i, v in enumerate(genotype):
            allele_to_id[pos][v] = i
            id_to_allele[pos][i] = v
        is_homozygous[pos] = len(set(genotype)) == 1
        phased[pos] = object() if is_phased else None
        change[pos] = _Change(bool(snv))
    reads = []
    for k, r in enumerate(data["reads"]):
        read = Read(f"read{k}", 0, 0, 0, 0, "", r["hp"], r["ps"])
        for pos, allele, quality in r["variants"]:
            read.add_variant(pos, allele, quality)
        reads.append(read)
    return dict(is_homozygous=is_homozygous, reads=reads, allele_to_id=allele_to_id, id_to_allele=id_to_allele, change=change, phased=phased,
                refseq=data["refseq"])


def canonical(votes, super_reads, components, skipped):
    """The results as plain lists that keep every order."""
    return dict(votes=[[int(pos), [[int(ps), int(h), int(s)] for (ps, h), s in vote.items()]] for pos, vote in votes.items()],
                super_reads=[[[int(v.position), int(v.allele), int(v.quality)] for v in read] for read in super_reads],
                components=[[int(pos), int(ps)] for pos, ps in components.items()], skipped=int(skipped))


def input_sha256(data):
    return hashlib.sha256(json.dumps(data, sort_keys=True, separators=(",", ":")).encode()).hexdigest()


# ---------------------------------------------------------------------------------------------- specs
HET, HOM, ALT12 = [0, 1], [1, 1], [1, 2]


def _read(ps, hp, variants):
    """ps, hp: the tags as the read carries them (the functions subtract 1)."""
    return dict(ps=ps, hp=hp, variants=[list(v) for v in variants])


def _explicit(name, variants, reads, only_indels=False, gap=70, cut=0, refseq="", expect_error=None):
    """variants: [(position, genotype vector, already phased, is SNV)]."""
    return dict(name=name, kind="explicit", only_indels=only_indels, gap_threshold=gap, cut_homopolymers=cut, expect_error=expect_error,
                data=dict(refseq=refseq, variants=[[p, list(g), bool(ph), bool(snv)] for p, g, ph, snv in variants], reads=reads))


def explicit_specs():
    specs = []
    A, B, C3 = 101, 201, 301   # PS tags
    plain = [(10, HET, False, True), (20, HET, False, False), (30, HET, False, True), (40, HET, False, False)]
    # ties between two phase sets: the one met first at the position wins, whichever read order
    specs.append(_explicit("tie_phasesets_a_first", plain, [_read(A, 1, [(10, 0, 7), (20, 1, 5)]), _read(B, 1, [(10, 0, 7), (20, 0, 5)]),
                                                            _read(B, 2, [(20, 0, 0)])], gap=0))
    specs.append(_explicit("tie_phasesets_b_first", plain, [_read(B, 2, [(10, 1, 7)]), _read(A, 1, [(10, 0, 3), (10, 0, 4)]), _read(C3, 1, [(10, 1, 7)])], gap=0))
    # tie between the two haplotypes of one phase set: haplotype 0, also where haplotype 1 got its votes first
    specs.append(_explicit("tie_haplotypes", plain, [_read(A, 2, [(10, 0, 6), (20, 0, 4)]), _read(A, 1, [(10, 0, 6), (20, 0, 4)]), _read(A, 1, [(30, 1, 9)]),
                                                     _read(A, 2, [(30, 1, 9)])], gap=0))
    # a phase set first met by a read that is later outvoted; it still orders the dict
    specs.append(_explicit("first_met_outvoted", plain, [_read(B, 1, [(10, 0, 2), (20, 0, 2)]), _read(A, 1, [(10, 0, 30), (20, 1, 30)]),
                                                         _read(A, 2, [(10, 1, 30), (30, 0, 9)]), _read(B, 2, [(30, 0, 9), (30, 1, 1)])], gap=0))
    # every combination of HP_tag - 1 in (-1, 0, 1, 2) and PS_tag - 1 below 0 or not
    combos = [_read(ps, hp, [(10, 0, 5 + hp + (ps > 0)), (20, 1, 3)]) for ps in (0, -5, A, B) for hp in (0, 1, 2, 3)]
    specs.append(_explicit("tags_every_combination", plain, combos, gap=0))
    specs.append(_explicit("only_skipped_and_ignored", plain, [_read(A, 3, [(10, 0, 5)]), _read(0, 3, [(10, 0, 5)]), _read(A, 0, [(10, 0, 5)]),
                                                               _read(A, 7, [(20, 0, 5)])], gap=0))
    # a homozygous position between heterozygous ones
    specs.append(_explicit("homozygous_between", [(10, HET, False, True), (20, HOM, False, True), (30, HET, False, True), (25, [0, 0], False, False)],
                           [_read(A, 1, [(10, 0, 5), (20, 1, 50), (25, 0, 9), (30, 1, 5)]), _read(A, 2, [(20, 1, 50), (30, 0, 4)])], gap=0))
    # already phased positions fail the gap threshold but stay; unphased ones go
    specs.append(_explicit("phased_stay_below_gap", [(10, HET, True, True), (20, HET, False, True), (30, HET, True, False), (40, HET, False, False)],
                           [_read(A, 1, [(10, 0, 5), (20, 0, 5), (30, 0, 5), (40, 0, 5)]), _read(A, 2, [(10, 0, 4), (20, 0, 4), (30, 0, 4), (40, 0, 4)]),
                            _read(B, 1, [(10, 1, 3), (20, 1, 3), (30, 1, 3), (40, 1, 3)])], gap=90))
    # 100 * fraction against the threshold: exactly equal (7 of 10 at 70), one unit below and above, and a fraction that is not a binary one
    at_gap = [(10, HET, False, False), (20, HET, False, False), (30, HET, False, False), (40, HET, False, False), (50, HET, False, False)]
    specs.append(_explicit("gap_exact", at_gap, [_read(A, 1, [(10, 0, 7), (20, 0, 69), (30, 0, 71), (40, 0, 7), (50, 0, 2)]),
                                                 _read(A, 2, [(10, 0, 3), (20, 0, 31), (30, 0, 29), (40, 0, 2), (50, 0, 1)]),
                                                 _read(B, 1, [(40, 1, 1)])], gap=70))
    specs.append(_explicit("gap_float_threshold", at_gap, [_read(A, 1, [(10, 0, 2), (20, 0, 1), (30, 0, 29)]), _read(A, 2, [(10, 0, 1), (20, 0, 2), (30, 0, 71)])],
                           gap=66.66666666666667))
    specs.append(_explicit("gap_100", at_gap, [_read(A, 1, [(10, 0, 5), (20, 0, 5)]), _read(A, 2, [(20, 0, 1)])], gap=100))
    # only_indels with SNVs and other variants, phased and not
    mixed = [(10, HET, False, True), (20, HET, False, False), (30, HET, True, True), (40, HET, True, False)]
    for flag in (True, False):
        specs.append(_explicit(f"only_indels_{int(flag)}", mixed, [_read(A, 1, [(10, 0, 9), (20, 1, 9), (30, 0, 9), (40, 1, 9)]), _read(A, 2, [(10, 1, 8), (40, 0, 1)])],
                               only_indels=flag, gap=50))
    # homopolymers longer than cut_homopolymers on both flanks: the filter drops nothing; cut_homopolymers = 0 switches it off
    ref = "ACGT" + "A" * 30 + "C" + "T" * 30 + "GATTACA" + "G" * 40
    homo = [(20, HET, False, False), (34, HET, False, False), (35, HET, False, True), (50, HET, False, False), (80, HET, False, False), (3, HET, False, False)]
    homo_reads = [_read(A, 1, [(3, 0, 5), (20, 0, 5), (34, 1, 6), (35, 0, 7), (50, 1, 8), (80, 0, 9)]), _read(A, 2, [(20, 1, 1), (50, 0, 2)])]
    for cut in (0, 1, 5, 29, 30, 100):
        specs.append(_explicit(f"homopolymer_cut_{cut}", homo, homo_reads, cut=cut, refseq=ref, gap=10))
    # a genotype vector [1, 2]: ids 0 / 1 stand for alleles 1 / 2
    specs.append(_explicit("genotype_1_2", [(10, ALT12, False, False), (20, HET, False, True), (30, [2, 1], False, False)],
                           [_read(A, 1, [(10, 1, 9), (20, 0, 9), (30, 1, 4)]), _read(A, 2, [(10, 2, 9), (20, 1, 8), (30, 1, 4)]), _read(A, 1, [(10, 2, 1), (30, 2, 9)])], gap=0))
    # the same position twice in one read
    specs.append(_explicit("position_twice", plain, [_read(A, 1, [(10, 0, 5), (10, 1, 3), (10, 0, 2), (20, 1, 1)]), _read(B, 2, [(20, 0, 1), (20, 0, 1), (10, 1, 4)])], gap=0))
    # negative and large qualities
    big = (1 << 31) - 1
    specs.append(_explicit("extreme_qualities", plain, [_read(A, 1, [(10, 0, big), (20, 0, -5), (30, 0, -(1 << 31)), (40, 0, -3)]),
                                                        _read(A, 1, [(10, 0, big), (20, 1, 2), (30, 1, -(1 << 31)), (40, 1, -3)]),
                                                        _read(B, 2, [(10, 0, big), (10, 1, big), (20, 0, -9), (40, 0, -7)])], gap=40))
    # no counted entry at all
    specs.append(_explicit("no_counted_entry", [(10, HOM, False, True), (20, HET, False, True)], [_read(A, 1, [(10, 1, 5)]), _read(A, 0, [(20, 0, 5)]),
                                                                                                   _read(0, 1, [(20, 0, 5)]), _read(A, 3, [(20, 1, 5)]), _read(A, 1, [])]))
    specs.append(_explicit("no_reads", plain, []))
    # errors
    specs.append(_explicit("error_zero_total", plain, [_read(A, 1, [(10, 0, 5), (20, 0, 0)]), _read(A, 2, [(20, 1, 0)])], gap=0, expect_error="ZeroDivisionError"))
    specs.append(_explicit("error_zero_total_cancels", plain, [_read(A, 1, [(10, 0, 5), (20, 0, 4)]), _read(B, 2, [(10, 1, 5), (10, 0, -10)])], gap=0,
                           expect_error="ZeroDivisionError"))
    specs.append(_explicit("error_unknown_allele", plain, [_read(A, 1, [(10, 0, 5)]), _read(A, 1, [(10, 2, 5)])], expect_error="KeyError"))
    specs.append(_explicit("error_unknown_position", plain, [_read(A, 1, [(10, 0, 5), (15, 0, 5)])], expect_error="KeyError"))
    # ... which the reference does not reach in a read that does not vote, nor (the allele) at a homozygous position
    specs.append(_explicit("unknown_in_ignored_reads", [(10, HET, False, True), (20, HOM, False, True)],
                           [_read(A, 0, [(15, 0, 5)]), _read(A, 3, [(10, 7, 5)]), _read(A, 1, [(20, 5, 5), (10, 1, 5)])], gap=0))
    return specs


def random_specs():
    specs = []

    def add(name, **kw):
        base = dict(name=name, kind="random", seed=2000 + len(specs), only_indels=False, gap_threshold=70, cut_homopolymers=0, expect_error=None, n_variants=40,
                    n_phasesets=3, n_reads=60, lengths=[0, 1, 2, 3, 5, 8, 13], quality=[1, 60], p_hom=0.15, p_phased=0.5, p_snv=0.6, p_error=0.15,
                    hp_tags=[0, 1, 1, 1, 2, 2, 2, 3], p_no_ps=0.1, p_alt12=0.1, p_twice=0.05)
        assert set(kw) <= set(base)
        base.update(kw)
        specs.append(base)

    for k in range(6):
        add(f"mixed_{k}", only_indels=bool(k & 1), gap_threshold=(0, 50, 70, 90, 100, 60.5)[k], cut_homopolymers=(0, 3, 0, 10, 1, 0)[k])
    for k in range(6):
        add(f"tie_heavy_{k}", quality=[1, 2], lengths=[1, 2, 2, 3, 4], n_phasesets=2 + k % 3, n_reads=80, n_variants=12, gap_threshold=(50, 34, 25)[k % 3])
    for n_ps in range(1, 9):
        add(f"phasesets_{n_ps}", n_phasesets=n_ps, n_variants=10, n_reads=30 + 10 * n_ps, lengths=[4, 6, 10], quality=[1, 9], gap_threshold=30)
    add("negative_qualities", quality=[-20, 30], gap_threshold=40)
    add("huge_qualities", quality=[(1 << 31) - 40, (1 << 31) - 1], lengths=[3, 9, 27])
    add("deep", n_variants=6, n_reads=400, lengths=[3, 4, 6], n_phasesets=6, gap_threshold=20)
    add("all_phased", p_phased=1.0, gap_threshold=100)
    add("none_phased_only_indels", p_phased=0.0, only_indels=True, gap_threshold=55)
    return specs


def all_specs():
    specs = explicit_specs() + random_specs()
    assert len({s["name"] for s in specs}) == len(specs)
    return specs


def materialize(spec):
    """The complete input of a case as plain data (what call_args builds the objects from)."""
    if spec["kind"] == "explicit":
        return spec["data"]
    rng = random.Random(spec["seed"])
    n_var = spec["n_variants"]
    positions = sorted(rng.sample(range(5, 5 + n_var * 20), n_var))
    variants = []
    for pos in positions:
        genotype = [1, 1] if rng.random() < spec["p_hom"] else ([1, 2] if rng.random() < spec["p_alt12"] else [0, 1])
        variants.append([pos, genotype, rng.random() < spec["p_phased"], rng.random() < spec["p_snv"]])
    tags = [rng.randrange(1, 1 << 40) for _ in range(spec["n_phasesets"])]
    truth = [[rng.randrange(2) for _ in range(n_var)] for _ in tags]   # per phase set: the id haplotype 0 carries
    reads = []
    for _ in range(spec["n_reads"]):
        length = min(rng.choice(spec["lengths"]), n_var)
        at = rng.randrange(n_var - length + 1)
        k = rng.randrange(len(tags))
        ps = rng.choice((0, -3)) if rng.random() < spec["p_no_ps"] else tags[k]
        hp = rng.choice(spec["hp_tags"])
        entries = []
        for i in range(at, at + length):
            ident = truth[k][i] ^ (hp & 1)
            if rng.random() < spec["p_error"]:
                ident ^= 1
            genotype = variants[i][1]
            entries.append([positions[i], genotype[ident], rng.randint(*spec["quality"])])
            if rng.random() < spec["p_twice"]:
                entries.append([positions[i], genotype[ident ^ 1], rng.randint(*spec["quality"])])
        reads.append(_read(ps, hp, entries))
    refseq = "".join(rng.choice("AAACGT") for _ in range(5 + n_var * 20 + 10))
    return dict(refseq=refseq, variants=variants, reads=reads)


def load_golden():
    with gzip.open(GOLDEN, "rb") as f:
        return json.loads(f.read().decode())


# ---------------------------------------------------------------------------------------------- array-level problems (device tests, benchmark)
def array_problem(runs, seed, n_phasesets=3, mean_read=12, quality=(1, 60), n_homozygous=3, p_idle_reads=0.2, ps_in_order=False, gap_threshold=60.0,
                  only_indels=False):
    """A whatshap_amd.haplotagphase.TagphaseProblem in which variant v gets exactly ``runs[v]`` voting entries (numpy generator ``seed``).
    The voting entries are shuffled and cut into reads of ``mean_read`` entries on average, every read with one of ``n_phasesets`` phase
    sets and a haplotype; ``ps_in_order``: the entries are not shuffled and the phase set follows the read's place (``n_phasesets`` stretches; four or fewer: they alternate), so
    the parts of a long run meet different phase sets.  ``n_homozygous`` more variants take entries that do not vote, and
    ``p_idle_reads`` more reads (hp of -1 or 2, or ps below 0) carry entries that do not vote either."""
    from whatshap_amd.haplotagphase import HOMOZYGOUS, PHASED, SNV, TagphaseProblem

    rng = np.random.default_rng(seed)
    runs = np.asarray(runs, dtype=np.int64)
    n_het = runs.size
    n_var = n_het + n_homozygous
    flags = rng.choice(np.array([0, PHASED, SNV, PHASED | SNV], dtype=np.uint8), size=n_var)
    flags[n_het:] |= HOMOZYGOUS
    pool = np.repeat(np.arange(n_het, dtype=np.int64), runs)
    if n_homozygous and pool.size:
        pool = np.concatenate([pool, rng.integers(n_het, n_var, size=max(1, pool.size // 20))])
    if not ps_in_order:
        rng.shuffle(pool)
    n_voting_reads = max(1, pool.size // mean_read) if pool.size else 0
    cuts = np.sort(rng.integers(0, pool.size + 1, size=max(n_voting_reads - 1, 0)))
    lengths = np.diff(np.concatenate([[0], cuts, [pool.size]])) if n_voting_reads else np.zeros(0, dtype=np.int64)
    tags = rng.integers(0, 1 << 40, size=n_phasesets, dtype=np.int64)
    if ps_in_order:
        ps = tags[(np.arange(lengths.size) * n_phasesets) // max(lengths.size, 1)] if n_phasesets > 4 else tags[np.arange(lengths.size) % n_phasesets]
    else:
        ps = tags[rng.integers(0, n_phasesets, size=lengths.size)]
    hp = rng.integers(0, 2, size=lengths.size).astype(np.int32)
    # idle reads: inserted between the voting ones
    n_idle = int(lengths.size * p_idle_reads) + (2 if p_idle_reads else 0)
    idle_len = rng.integers(0, 2 * mean_read, size=n_idle) if n_var else np.zeros(n_idle, dtype=np.int64)
    idle_ps = np.where(rng.random(n_idle) < 0.3, -1 - rng.integers(0, 3, size=n_idle), tags[rng.integers(0, n_phasesets, size=n_idle)])
    idle_hp = np.where(idle_ps < 0, rng.integers(-1, 4, size=n_idle), rng.choice(np.array([-1, 2, 3]), size=n_idle)).astype(np.int32)
    where = np.sort(rng.integers(0, lengths.size + 1, size=n_idle))
    order = np.argsort(np.concatenate([np.arange(lengths.size) * 2 + 1, where * 2]), kind="stable")
    all_len = np.concatenate([lengths, idle_len])[order]
    all_ps = np.concatenate([ps, idle_ps])[order]
    all_hp = np.concatenate([hp, idle_hp])[order]
    is_idle = np.concatenate([np.zeros(lengths.size, dtype=bool), np.ones(n_idle, dtype=bool)])[order]
    read_ptr = np.zeros(all_len.size + 1, dtype=np.uint64)
    np.cumsum(all_len, out=read_ptr[1:])
    n_entries = int(read_ptr[-1])
    entry_variant = np.zeros(n_entries, dtype=np.int64)
    idle_entries = np.repeat(is_idle, all_len)
    entry_variant[~idle_entries] = pool
    entry_variant[idle_entries] = rng.integers(0, n_var, size=int(idle_entries.sum()))
    entry_id = rng.integers(0, 2, size=n_entries)
    entry_quality = rng.integers(quality[0], quality[1] + 1, size=n_entries, dtype=np.int64)
    return TagphaseProblem(flags, read_ptr, entry_variant, entry_id, entry_quality, all_ps, all_hp, gap_threshold, only_indels)


def heavy_tail_runs(n_variants, seed, mean=30, tail=0.001, tail_max=20000):
    """Coverage per variant: geometric around ``mean`` with zeros and ones, and a heavy tail of a few very deep variants."""
    rng = np.random.default_rng(seed)
    runs = rng.geometric(1.0 / mean, size=n_variants) - 1
    deep = rng.random(n_variants) < tail
    runs[deep] = rng.integers(100, tail_max, size=int(deep.sum()))
    return runs


def bench_problem(n_reads=2_000_000, seed=7, n_variants=1_000_000, mean_length=30):
    """The problem of scripts/gpu_haplotagphase_bench.py: a deep long-read chromosome.  ``n_reads`` reads list ``mean_length`` consecutive
    variants on average (geometric, a few of thousands) from a random place; phase sets cover stretches of 20 000 variants (a read has the
    one of its first variant); 4 % of the reads carry no usable tags; 10 % of the variants are homozygous, 60 % phased already, 85 % SNVs;
    the ids follow the read's haplotype with 15 % errors."""
    from whatshap_amd.haplotagphase import HOMOZYGOUS, PHASED, SNV, TagphaseProblem

    rng = np.random.default_rng(seed)
    lengths = rng.geometric(1.0 / mean_length, size=n_reads) - 1
    long_ones = rng.random(n_reads) < 0.0002
    lengths[long_ones] = rng.integers(100, 20000, size=int(long_ones.sum()))
    lengths = np.minimum(lengths, n_variants)
    read_ptr = np.zeros(n_reads + 1, dtype=np.uint64)
    np.cumsum(lengths, out=read_ptr[1:])
    n_entries = int(read_ptr[-1])
    first = rng.integers(0, n_variants - lengths + 1)
    read_of = np.repeat(np.arange(n_reads), lengths)
    entry_variant = first[read_of] + (np.arange(n_entries) - read_ptr[:-1].astype(np.int64)[read_of])
    flags = (np.where(rng.random(n_variants) < 0.1, HOMOZYGOUS, 0) | np.where(rng.random(n_variants) < 0.6, PHASED, 0)
             | np.where(rng.random(n_variants) < 0.85, SNV, 0)).astype(np.uint8)
    ps = (first // 20000) * 20000 + 1000
    hp = rng.integers(0, 2, size=n_reads).astype(np.int32)
    untagged = rng.random(n_reads) < 0.04
    hp[untagged] = rng.choice(np.array([-1, 2], dtype=np.int32), size=int(untagged.sum()))
    truth = rng.integers(0, 2, size=n_variants)
    entry_id = truth[entry_variant] ^ (hp[read_of] & 1) ^ (rng.random(n_entries) < 0.15)
    entry_quality = rng.integers(1, 61, size=n_entries, dtype=np.int64)
    return TagphaseProblem(flags, read_ptr, entry_variant, entry_id, entry_quality, ps, hp, 70.0, True)
