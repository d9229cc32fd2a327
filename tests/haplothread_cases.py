"""Seeded cases of the polyphase threading DP (whatshap_amd.polythread.thread_batch), shared by tests/golden/make_haplothread_golden.py
(which records what the reference's HaploThreader makes of them) and by tests/test_haplothread_host.py / tests/test_gpu_haplothread.py.

A case is a dict of plain lists: ``name``, ``ploidy``, ``cov_map`` (per position the listed cluster ids), ``depths`` (per position a list
of [cluster, total depth] rows: every listed cluster has one, further rows may exist), ``switch_cost``, ``affine_switch_cost``,
``max_gap``, ``block_starts``, and the flags ``tie_heavy`` (check (E), path == reference path, is not asked of it) and ``small`` (the
golden file also records the coverage cost of every tuple).
"""
import gzip
import json
import os
import random

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "haplothread_cases.json.gz")
PLOIDIES = (2, 3, 4, 5, 6)
RANDOM_PER_PLOIDY = {2: 12, 3: 12, 4: 12, 5: 12, 6: 6}


def enumerate_tuples(ploidy, n):
    """The tuples of ``ploidy`` local ids out of n in the order the threader enumerates them: non-increasing, the first slot fastest."""
    out, v = [], [0] * ploidy
    while v[ploidy - 1] < n:
        out.append(list(v))
        v[0] += 1
        for i in range(1, ploidy):
            if v[i - 1] >= n:
                v[i] += 1
        for i in range(ploidy - 1, 0, -1):
            if v[i - 1] >= n:
                v[i - 1] = v[i]
    return out


def case(name, ploidy, cov_map, depths, switch_cost=12.0, affine_switch_cost=3.0, max_gap=10, block_starts=(0,), tie_heavy=False, small=False):
    return {"name": name, "ploidy": ploidy, "cov_map": [list(map(int, c)) for c in cov_map], "depths": [[[int(c), int(d)] for c, d in rows] for rows in depths],
            "switch_cost": switch_cost, "affine_switch_cost": affine_switch_cost, "max_gap": max_gap, "block_starts": list(block_starts), "tie_heavy": tie_heavy,
            "small": small}


def random_case(seed, ploidy, n_pos=None, width=None, lo=5, hi=80, **kw):
    """Clusters of a pool of ploidy + 4 live over intervals of positions; a position lists those alive (at most ``width``, default
    min(ploidy + 2, 8)), in shuffled order now and then; the depth of a cluster wanders around a level drawn from lo .. hi."""
    rng = random.Random(seed)
    n_pos = n_pos or rng.randint(12, 40)
    width = width or min(ploidy + 2, 8)
    pool = list(range(3, 3 + ploidy + 4))
    level = {c: rng.randint(lo, hi) for c in pool}
    alive = set(rng.sample(pool, rng.randint(max(2, width - 2), width)))
    cov_map, depths = [], []
    for x in range(n_pos):
        if rng.random() < 0.25 and len(alive) > 1:
            alive.discard(rng.choice(sorted(alive)))
        if rng.random() < 0.3 and len(alive) < width:
            alive.add(rng.choice([c for c in pool if c not in alive]))
        listed = sorted(alive)
        if rng.random() < 0.2:
            rng.shuffle(listed)
        rows = [[c, max(1, level[c] + rng.randint(-level[c] // 5, level[c] // 5))] for c in listed]
        extra = [c for c in pool if c not in alive]
        if extra and rng.random() < 0.3:
            rows.append([rng.choice(extra), rng.randint(1, 9)])   # a row of a cluster the position does not list
        rng.shuffle(rows)
        cov_map.append(listed)
        depths.append(rows)
    return case(kw.pop("name", f"random_p{ploidy}_s{seed}"), ploidy, cov_map, depths, **kw)


def full_case(name, ploidy, n_clusters, n_pos, seed, **kw):
    """Every position lists the same n_clusters clusters: full columns of C(n_clusters + ploidy - 1, ploidy) tuples."""
    rng = random.Random(seed)
    ids = [10 * c + 1 for c in range(n_clusters)]
    lo, hi = kw.pop("lo", 2), kw.pop("hi", 9)
    cov_map = [ids for _ in range(n_pos)]
    depths = [[[c, rng.randint(lo, hi)] for c in ids] for _ in range(n_pos)]
    return case(name, ploidy, cov_map, depths, **kw)


def random_cases():
    return [random_case(1000 * p + k, p) for p in PLOIDIES for k in range(RANDOM_PER_PLOIDY[p])]


def shape_cases():
    out = []
    # the widest column of every ploidy, nothing pruned (small depths), and a position with one cluster in the middle
    for p, n in ((2, 4), (3, 5), (4, 6), (5, 7), (6, 8)):
        c = full_case(f"full_{p}_{n}", p, n, 4, seed=p, small=p <= 4, max_gap=0)
        c["cov_map"][2] = c["cov_map"][2][:1]
        out.append(c)
    out.append(full_case("full_6_8_shallow", 6, 8, 3, seed=66, lo=1, hi=3))   # (most of the 1 716 tuples stay: columns wider than a workgroup)
    out.append(full_case("full_6_8_wide_depths", 6, 8, 3, seed=66, lo=5, hi=80))
    # sections of 1 and 2 positions, several sections
    out.append(random_case(71, 3, n_pos=9, block_starts=(0, 1, 3, 4, 4, 8), small=True, name="sections"))
    out.append(random_case(72, 2, n_pos=1, small=True, name="one_position"))
    out.append(random_case(73, 4, n_pos=2, small=True, name="two_positions"))
    # no cluster survives from one column to the next: no equivalent predecessor, every slot switches
    out.append(case("disjoint_columns", 3, [[1, 2, 3], [4, 5, 6], [1, 2, 3], [7]], [[[1, 30], [2, 20], [3, 9]], [[4, 30], [5, 21], [6, 8]], [[1, 31], [2, 19], [3, 10]], [[7, 50]]],
                    small=True))
    # re-added clusters: listed with a depth row of 0; and a cluster of depth 0 in its whole window
    out.append(case("readded_empty_rows", 2, [[1, 2], [1, 2, 3], [1, 2, 3], [2, 3], [2, 3, 9]],
                    [[[1, 20], [2, 22]], [[1, 19], [2, 0], [3, 7]], [[1, 0], [2, 25], [3, 0]], [[2, 24], [3, 30]], [[2, 20], [3, 28], [9, 0]]], max_gap=2, small=True))
    # windows: gap 0 (the reference's window then reaches back to position 0), 1, 10, larger than the problem
    for gap in (0, 1, 10, 1000, 0xFFFFFFFF):
        out.append(random_case(80 + gap % 7, 3, n_pos=14, max_gap=gap, small=True, name=f"gap_{gap}"))
    # pruning: one dominant cluster leaves one tuple per column; depths of a few reads prune nothing
    out.append(case("all_but_one_pruned", 2, [[1, 2]] * 3, [[[1, 300], [2, 0]], [[1, 280], [2, 0]], [[1, 310], [2, 0]]], max_gap=0, small=True))
    out.append(case("none_pruned", 2, [[1, 2, 3]] * 3, [[[1, 2], [2, 1], [3, 3]], [[1, 1], [2, 3], [3, 2]], [[1, 3], [2, 2], [3, 1]]], max_gap=0, small=True))
    # costs
    out.append(random_case(91, 3, affine_switch_cost=0.0, small=True, name="affine_zero"))
    out.append(random_case(92, 4, switch_cost=0.5, affine_switch_cost=0.25, name="costs_half_quarter"))
    out.append(random_case(93, 2, switch_cost=4.0, affine_switch_cost=1.0, small=True, name="pipeline_costs"))
    # tie-heavy
    out.append(full_case("equal_coverages", 3, 4, 8, seed=1, lo=20, hi=20, tie_heavy=True, small=True))
    zero = full_case("zero_coverage_position", 2, 3, 5, seed=2, lo=10, hi=40, tie_heavy=True, small=True, max_gap=0)
    zero["depths"][0] = [[c, 0] for c, _ in zero["depths"][0]]
    zero["depths"][3] = [[c, 0] for c, _ in zero["depths"][3]]
    out.append(zero)
    out.append(random_case(94, 3, switch_cost=0.0, affine_switch_cost=3.0, tie_heavy=True, small=True, name="switch_cost_zero"))
    out.append(random_case(95, 3, switch_cost=0.0, affine_switch_cost=0.0, tie_heavy=True, small=True, name="all_costs_zero"))
    out.append(random_case(96, 3, n_pos=3000, tie_heavy=True, name="long_section"))
    return out


def all_cases():
    return random_cases() + shape_cases()


def arrays_of(c):
    """(cov_ptr, cov_cluster, pc_ptr, pc_cluster, pc_total) of a case."""
    cov_ptr = np.zeros(len(c["cov_map"]) + 1, dtype=np.uint64)
    np.cumsum([len(x) for x in c["cov_map"]], out=cov_ptr[1:])
    pc_ptr = np.zeros(len(c["depths"]) + 1, dtype=np.uint64)
    np.cumsum([len(x) for x in c["depths"]], out=pc_ptr[1:])
    cov = np.asarray([g for x in c["cov_map"] for g in x], dtype=np.uint32)
    rows = [r for x in c["depths"] for r in x]
    return cov_ptr, cov, pc_ptr, np.asarray([r[0] for r in rows], dtype=np.uint32), np.asarray([r[1] for r in rows], dtype=np.uint32)


def dicts_of(c):
    """(cov_map, allele_depths) in the reference's forms: the depth of a row as one allele's."""
    return [list(x) for x in c["cov_map"]], [{cid: ({0: d} if d else {}) for cid, d in rows} for rows in c["depths"]]


def sections_of(c):
    n, starts = len(c["cov_map"]), c["block_starts"]
    ends = list(starts[1:]) + [n]
    return [(s, e) for s, e in zip(starts, ends) if e > s]


def load_golden():
    with gzip.open(GOLDEN, "rb") as f:
        return json.loads(f.read().decode())


# ---------------------------------------------------------------------------------------------- the benchmark's inputs
def bench_problem(ploidy, n_pos, seed):
    """One section of n_pos positions: ploidy + 2 clusters listed at every position, depths wandering around levels of 5 .. 80."""
    rng = np.random.default_rng(seed)
    n = ploidy + 2
    level = rng.integers(5, 81, size=n)
    depth = np.maximum(1, level[None, :] + rng.integers(-8, 9, size=(n_pos, n))).astype(np.uint32)
    ptr = np.arange(n_pos + 1, dtype=np.uint64) * n
    ids = np.tile(np.arange(n, dtype=np.uint32), n_pos)
    return ptr, ids, ptr.copy(), ids.copy(), depth.reshape(-1)


# ---------------------------------------------------------------------------------------------- the checks both test files run
def f32(hex_string):
    return np.float32(float.fromhex(hex_string))


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def problem_of(c, **kw):
    from whatshap_amd import polythread

    return polythread.ThreaderProblem(*arrays_of(c), c["ploidy"], c["switch_cost"], c["affine_switch_cost"], c["max_gap"], c["block_starts"],
                                      want_costs=c.get("small", False), **kw)


def path_cost_under_recurrence(c, paths, path_cost, start, end):
    """(score + switch) + cov over one section, in float: switch = float(switch_cost k + affine (k > 0)), k the slots that change cluster
    under the best matching of the two tuples."""
    from collections import Counter

    P = c["ploidy"]
    score = np.float32(np.float32(0.0) + path_cost[start])
    for x in range(start + 1, end):
        common = sum((Counter(paths[x - 1]) & Counter(paths[x])).values())
        k = P - common
        switch = np.float32(c["switch_cost"] * k + c["affine_switch_cost"] * (k > 0))
        score = np.float32(np.float32(score + switch) + path_cost[x])
    return score


def check_case(rec, res):
    """Checks (A) - (E) of one recorded case against one ThreadingResult.  Returns whether every section had ambiguous == 0."""
    P, cov_map = rec["ploidy"], rec["cov_map"]
    n_pos = len(cov_map)
    sections = sections_of(rec)
    paths = res.paths.tolist()
    # (C)
    assert res.paths.shape == (n_pos, P)
    for x in range(n_pos):
        assert set(paths[x]) <= set(cov_map[x]), (rec["name"], x)
    assert res.section_first.tolist() == [s for s, _ in sections] and len(res.score) == len(sections) == len(res.ambiguous)
    # (D)
    assert res.smoothed.tolist() == rec["smoothed"], rec["name"]
    if rec.get("small"):
        recorded = np.asarray([float.fromhex(h) for position in rec["all_costs"] for h in position], dtype=np.float32)
        assert res.all_costs.size == recorded.size and (bits(res.all_costs) == bits(recorded)).all(), rec["name"]
    ref_cost = np.asarray([float.fromhex(h) for h in rec["path_cost"]], dtype=np.float32)
    same_tuple = np.asarray([sorted(paths[x]) == sorted(rec["path"][x]) for x in range(n_pos)])
    assert (bits(res.path_cost)[same_tuple] == bits(ref_cost)[same_tuple]).all(), rec["name"]
    unambiguous = True
    for k, (start, end) in enumerate(sections):
        optimum = f32(rec["optimum"][k])
        # (A)
        assert bits(res.score[k]) == bits(optimum), (rec["name"], k, float(res.score[k]), float(optimum))
        # (B)
        mine = path_cost_under_recurrence(rec, paths, res.path_cost, start, end)
        assert bits(mine) == bits(optimum), (rec["name"], k, float(mine), float(optimum))
        # (E)
        if res.ambiguous[k] == 0:
            assert paths[start:end] == rec["path"][start:end], (rec["name"], k)
        else:
            unambiguous = False
    return unambiguous
