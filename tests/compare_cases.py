"""Cases of comparing polyploid phasings (whatshap_amd.compare), shared by tests/golden/make_compare_golden.py -- which records what the
reference computes for them -- and by the tests, which read the recording.  Pure Python and numpy, seeded; nothing here needs the
reference or the library.

A case is a dict: ``name``, ``ploidy``, ``phasing0`` and ``phasing1`` (one string over 0-9 per haplotype) and ``costs``, the
[switch_cost, flip_cost] pairs the switch/flip program is run with.  Every case is also run as a whole block (compare_block) and with the
switch-error cost over its matching positions.

The shapes are the smallest at which each mechanism can go wrong (see all_cases()): 2, 6, 24, 120 and 720 states -- below a wave, across
waves, and 720 rows on 256 lanes with a ragged tail --, 1, 2 and 3 positions, 64, 65 and about 90; the ploidy-6 cases stay at or below 70.
"""
import itertools
import os
import random

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COSTS = [[1, 1], [2, 1], [1, 3], [0.5, 0.25]]


def arrays(case):
    """(phasing0, phasing1) as int arrays [n_pos][ploidy]."""
    return tuple(np.array([[int(c) for c in hap] for hap in case[key]], dtype=np.int64).reshape(case["ploidy"], -1).T for key in ("phasing0", "phasing1"))


def matching_positions(p0, p1):
    return [i for i in range(len(p0)) if sorted(p0[i].tolist()) == sorted(p1[i].tolist())]


def switch_error_cost(case):
    return 2 * len(case["phasing0"][0]) * case["ploidy"] + 1


_ORACLE = {}   # computed once per (input, costs), shared by the tests of a session


def dense_oracle(p0, p1, switch_cost=1, flip_cost=1):
    """(total, switches, flips) of the canonical split (_dense_oracle), computed once per input and cost pair."""
    key = (p0.shape, p0.tobytes(), p1.tobytes(), float(switch_cost), float(flip_cost))
    if key not in _ORACLE:
        _ORACLE[key] = _dense_oracle(np.asarray(p0, dtype=np.int64), np.asarray(p1, dtype=np.int64), switch_cost, flip_cost)
    return _ORACLE[key]


def _dense_oracle(p0, p1, switch_cost, flip_cost):
    """The canonical split: (total, switches, flips) of the path that minimises the pair (total, flips) over a dense k! x k! transition;
    among equals numpy's argmin takes the lowest rank.  p0, p1: [n_pos][ploidy], n_pos >= 1.  (One position: the program's own answer,
    switches = 0; the reference's ploidy - 1 there is not part of the program.)"""
    perms = np.array(list(itertools.permutations(range(p0.shape[1]))))
    D = (perms[:, None, :] != perms[None, :, :]).sum(-1)           # [r][q] places in which two permutations differ
    F = (p0[:, perms] != p1[:, None, :]).sum(-1)                   # [position][r] alleles that disagree under r
    score, flips, switches = flip_cost * F[0].astype(np.float64), F[0].copy(), np.zeros(len(perms), dtype=np.int64)
    rows = np.arange(len(perms))
    for c in range(1, len(p0)):
        cand = score[None, :] + switch_cost * D.astype(np.float64)
        best = cand.min(axis=1)
        q = np.where(cand == best[:, None], flips[None, :], np.iinfo(np.int64).max).argmin(axis=1)
        score, flips, switches = best + flip_cost * F[c], flips[q] + F[c], switches[q] + D[rows, q]
    end = min(rows.tolist(), key=lambda r: (score[r], flips[r], r))
    return float(score[end]), int(switches[end]), int(flips[end])


def min_hamming_sum(p0, p1):
    perms = np.array(list(itertools.permutations(range(p0.shape[1]))))
    return int((p0[:, perms] != p1[:, None, :]).sum(axis=(0, 2)).min()) if len(p0) else 0


# ---------------------------------------------------------------------------------------------- generators
def _strings(cols):
    return ["".join(str(a) for a in hap) for hap in np.asarray(cols).T.tolist()] if len(cols) else []


def _case(name, ploidy, p0, p1, costs=None):
    s0, s1 = _strings(p0), _strings(p1)
    if not s0:
        s0, s1 = [""] * ploidy, [""] * ploidy
    return dict(name=name, ploidy=ploidy, phasing0=s0, phasing1=s1, costs=[list(c) for c in (costs or COSTS)])


def _truth(rng, ploidy, n_pos, n_alleles=2, hom_rate=0.15):
    return [[rng.randrange(n_alleles)] * ploidy if rng.random() < hom_rate else [rng.randrange(n_alleles) for _ in range(ploidy)] for _ in range(n_pos)]


def planted(name, seed, ploidy, n_pos, n_alleles=2, switch_rate=0.08, flip_rate=0.05, geno_rate=0.05, start=None, costs=None):
    """phasing1 random; phasing0 the same haplotypes under a permutation that changes at planted switches, with planted flips (two
    haplotypes exchange their alleles: the genotype stays) and planted genotype errors (one allele replaced)."""
    rng = random.Random(seed)
    p1 = _truth(rng, ploidy, n_pos, n_alleles)
    perm = list(start) if start else list(range(ploidy))
    p0 = []
    for x in range(n_pos):
        if x and rng.random() < switch_rate:
            i, j = rng.sample(range(ploidy), 2)
            perm[i], perm[j] = perm[j], perm[i]
        col = [0] * ploidy
        for i in range(ploidy):
            col[perm[i]] = p1[x][i]     # phasing0[perm[i]] == phasing1[i]
        if rng.random() < flip_rate:
            i, j = rng.sample(range(ploidy), 2)
            col[i], col[j] = col[j], col[i]
        if rng.random() < geno_rate:
            col[rng.randrange(ploidy)] = rng.randrange(n_alleles)
        p0.append(col)
    return _case(name, ploidy, p0, p1, costs)


def permuted(name, seed, ploidy, n_pos, perm):
    """phasing0 a fixed non-identity permutation of phasing1: the cost is 0 and the end state is not rank 0."""
    return planted(name, seed, ploidy, n_pos, switch_rate=0.0, flip_rate=0.0, geno_rate=0.0, start=perm)


def duplicates(name, seed, ploidy, n_pos):
    """Every haplotype the same sequence: every permutation ties at every step."""
    rng = random.Random(seed)
    row = [rng.randrange(2) for _ in range(n_pos)]
    other = [a ^ (rng.random() < 0.1) for a in row]
    return _case(name, ploidy, [[a] * ploidy for a in row], [[a] * ploidy for a in other])


def all_equal_columns(name, ploidy, n_pos):
    return _case(name, ploidy, [[1] * ploidy] * n_pos, [[1] * ploidy] * n_pos)


def no_match(name, seed, ploidy, n_pos):
    """No position with matching genotypes: phasing0 carries one more 1 than phasing1 everywhere."""
    rng = random.Random(seed)
    p1 = [[0] * ploidy for _ in range(n_pos)]
    p0 = []
    for col in p1:
        for i in rng.sample(range(ploidy), rng.randrange(0, ploidy - 1)):
            col[i] = 1
        c = list(col)
        c[c.index(0)] = 1
        rng.shuffle(c)
        p0.append(c)
    return _case(name, ploidy, p0, p1)


def one_match(name, seed, ploidy, n_pos, at):
    """Exactly one position with matching genotypes."""
    case = no_match(name, seed, ploidy, n_pos)
    p0, p1 = arrays(case)
    p0[at] = p1[at][::-1]
    return _case(name, ploidy, p0.tolist(), p1.tolist())


def all_cases():
    cases = []
    for ploidy, sizes in ((2, (1, 2, 3, 64, 65, 90)), (3, (1, 2, 3, 64, 65, 90)), (4, (1, 2, 3, 64, 65, 91)), (5, (1, 2, 3, 64, 65, 89)), (6, (1, 2, 3, 64, 65, 70))):
        for n_pos in sizes:
            cases.append(planted(f"planted_p{ploidy}_n{n_pos}", 100 * ploidy + n_pos, ploidy, n_pos, switch_rate=0.1 if n_pos > 3 else 0.5,
                                 flip_rate=0.06 if n_pos > 3 else 0.4))
    cases += [permuted("permuted_p3", 1, 3, 40, [1, 2, 0]), permuted("permuted_p4", 2, 4, 33, [3, 0, 2, 1]), permuted("permuted_p5", 3, 5, 20, [4, 3, 2, 1, 0]),
              permuted("permuted_p6", 4, 6, 24, [5, 0, 4, 1, 3, 2])]
    cases += [duplicates("duplicates_p3", 5, 3, 30), duplicates("duplicates_p4", 6, 4, 30), duplicates("duplicates_p6", 7, 6, 12)]
    cases += [all_equal_columns("all_equal_p4", 4, 17), all_equal_columns("all_equal_p6", 6, 9)]
    cases += [planted("alleles_0_to_3_p3", 8, 3, 50, n_alleles=4), planted("alleles_0_to_3_p4", 9, 4, 66, n_alleles=4, geno_rate=0.15),
              planted("alleles_0_to_3_p6", 10, 6, 31, n_alleles=4)]
    cases += [no_match("no_match_p3", 11, 3, 12), no_match("no_match_p5", 12, 5, 7), one_match("one_match_p3", 13, 3, 12, 4), one_match("one_match_p4", 14, 4, 9, 0),
              one_match("one_match_p6", 15, 6, 5, 4)]
    cases += [planted("all_match_p4", 16, 4, 48, geno_rate=0.0), planted("all_match_p5", 17, 5, 37, geno_rate=0.0, flip_rate=0.12)]
    cases += [planted("many_errors_p4", 18, 4, 80, switch_rate=0.3, flip_rate=0.3, geno_rate=0.2), planted("many_errors_p5", 19, 5, 60, switch_rate=0.3, flip_rate=0.3),
              planted("many_errors_p6", 20, 6, 40, switch_rate=0.3, flip_rate=0.3, geno_rate=0.1)]
    assert 40 <= len(cases) <= 60 and len({c["name"] for c in cases}) == len(cases)
    assert all(len(c["phasing0"][0]) < 100 and (c["ploidy"] < 6 or len(c["phasing0"][0]) <= 70) for c in cases)
    return cases


def medium_cases():
    """Ploidy 6 with 300 positions and ploidy 5 with 1 000 (device against host twin and dense_oracle; the reference was not run on them)."""
    return [planted("medium_p6", 31, 6, 300, switch_rate=0.05, flip_rate=0.05), planted("medium_p5", 32, 5, 1000, n_alleles=3, switch_rate=0.04, flip_rate=0.04)]


def bench_block(seed, ploidy=6, n_pos=500):
    """A block of the benchmark (scripts/gpu_compare_bench.py, profiles/compare): (phasing0, phasing1) as uint8 [n_pos][ploidy]."""
    p0, p1 = arrays(planted("bench", seed, ploidy, n_pos, switch_rate=0.02, flip_rate=0.02, geno_rate=0.02))
    return p0.astype(np.uint8), p1.astype(np.uint8)


def load_golden():
    import gzip
    import json

    with gzip.open(os.path.join(ROOT, "tests", "golden", "compare_cases.json.gz"), "rt") as f:
        return json.load(f)


# ---------------------------------------------------------------------------------------------- checks
def jobs_of(case, want_path=True):
    """The jobs of a recorded case for whatshap_amd.compare.switch_flips_batch: one per cost pair over all positions, then the switch-error
    job over the matching positions."""
    from whatshap_amd.compare import CompareJob

    jobs = [CompareJob(case["phasing0"], case["phasing1"], sc, fc, want_path=want_path) for sc, fc in case["costs"]]
    jobs.append(CompareJob(case["phasing0"], case["phasing1"], 1, switch_error_cost(case), matched_only=True, want_path=want_path))
    return jobs


def check_path(p0, p1, positions, switch_cost, flip_cost, res):
    """The returned path is valid: every entry is a permutation, the per-column switches and flipped haplotypes recomputed from it are the
    returned ones and sum to the returned counts, and its cost is the total."""
    k = p0.shape[1]
    assert res.positions.tolist() == list(positions) and len(res.perms) == len(positions) == res.n_visited
    ranks = {perm: r for r, perm in enumerate(itertools.permutations(range(k)))}
    switches = flips = 0
    for v, x in enumerate(positions):
        perm = res.perms[v].tolist()
        assert sorted(perm) == list(range(k)) and ranks[tuple(perm)] == int(res.ranks[v])
        flipped = [int(p0[x][perm[i]] != p1[x][i]) for i in range(k)]
        assert res.flipped[v].tolist() == flipped
        d = sum(a != b for a, b in zip(perm, res.perms[v - 1].tolist())) if v else (k - 1 if len(positions) == 1 else 0)
        assert int(res.switches_in_column[v]) == d
        switches += d
        flips += sum(flipped)
    assert (switches, flips) == (res.switches, res.flips)
    if len(positions) != 1:
        assert switch_cost * switches + flip_cost * flips == res.total


def check_against_recording(case, results):
    """The results of jobs_of(case) against what the reference recorded and against dense_oracle.
    Identical to the reference: the total (switch_cost * switches + flip_cost * flips of its raw counts: every cost of the cases is exact
    in double), the switch-error count, the matching positions, the minimum Hamming distance, the result for one position / one match.
    Equal to dense_oracle: switches and flips (the canonical split); flips at most the reference's."""
    p0, p1 = arrays(case)
    n_pos, k = p0.shape
    matching = matching_positions(p0, p1)
    assert matching == case["ref"]["matching_pos"]
    assert len(results) == len(case["costs"]) + 1
    for (sc, fc), rec, res in zip(case["costs"], case["ref"]["runs"], results):
        assert (res.n_matched, res.n_visited) == (len(matching), n_pos)
        assert res.min_hamming_sum == min_hamming_sum(p0, p1)
        # (the reference's diploid branch truncates the mean to an int)
        assert (res.min_hamming_sum // 2 if k == 2 else res.min_hamming_sum / float(k)) == case["ref"]["block"]["hamming"]
        if n_pos == 1:   # the reference's one-position result, its flips the minimum
            assert [res.switches, res.flips] == rec["raw"] == [k - 1, res.min_hamming_sum] and res.total == fc * res.flips
        else:
            total, switches, flips = dense_oracle(p0, p1, sc, fc)
            assert res.total == total == sc * rec["raw"][0] + fc * rec["raw"][1], (case["name"], sc, fc)
            assert (res.switches, res.flips) == (switches, flips) and res.flips <= rec["raw"][1], (case["name"], sc, fc)
        if res.positions is not None:
            check_path(p0, p1, range(n_pos), sc, fc, res)
    res = results[-1]
    assert (res.n_matched, res.n_visited, res.flips) == (len(matching), len(matching), 0)
    assert res.switches == round(case["ref"]["switch_errors"] * k) and res.switches / k == case["ref"]["switch_errors"]
    if len(matching) == 0:
        assert (res.total, res.switches, res.min_hamming_sum) == (0.0, 0, 0)
    elif len(matching) == 1:
        assert res.switches == k - 1
    else:
        assert (res.total, res.switches, res.flips) == dense_oracle(p0[matching], p1[matching], 1, switch_error_cost(case))
    if res.positions is not None:
        check_path(p0, p1, matching, 1, switch_error_cost(case), res)
