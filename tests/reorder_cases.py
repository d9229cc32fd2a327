"""Cases of polyphase reordering (whatshap_amd.reorder), shared by tests/golden/make_reorder_golden.py -- which records what the reference
computes for them -- and by the tests, which read the recording.  Pure Python, seeded; nothing here needs the reference or the library.

A case is a dict: ``ploidy``, ``n_pos``, ``error_rate``, ``reads`` (per read a list of [local position, allele]; every position is listed
by some read, so local position p is genome position 100 + 7 p of the matrix), ``haplotypes`` [ploidy][n_pos], ``threads`` [n_pos][ploidy],
``clustering`` (lists of read ids) and ``breakpoints`` ([position, sorted affected haplotypes]).

The shapes are the smallest at which each mechanism can go wrong (see all_cases()); the one size taken from the code is the number of
reads one LDS tile of the permutation kernel holds, PR_READ_TILE of csrc/polyreorder.h.
"""
import os
import random
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read_tile():
    text = open(os.path.join(ROOT, "whatshap_amd", "csrc", "polyreorder.h")).read()
    return int(re.search(r"PR_READ_TILE = (\d+);", text).group(1))


def global_position(p):
    return 100 + 7 * p


def find_breakpoints(threads):
    """What reorder.find_breakpoints yields (the golden generator checks this against the reference's own)."""
    out = []
    ploidy = len(threads[0])
    for i in range(1, len(threads)):
        left = {threads[i - 1][j] for j in range(ploidy) if threads[i - 1][j] != threads[i][j]}
        affected = [j for j in range(ploidy) if threads[i - 1][j] in left]
        if len(affected) >= 2:
            out.append([i, affected])
    return out


def _finish(name, rng, ploidy, n_pos, haps, threads, reads, cluster_of, n_clusters, breakpoints, error_rate=0.07):
    """Covers every position, forms the clustering (reads in shuffled order: the order within a cluster matters) and the dict."""
    covered = {p for row in reads for p, _ in row}
    for p in range(n_pos):
        if p not in covered:   # (a single-position read spans no breakpoint)
            reads.append([[p, 0]])
            cluster_of.append(rng.randrange(n_clusters))
    order = list(range(len(reads)))
    rng.shuffle(order)
    clustering = [[] for _ in range(n_clusters)]
    for r in order:
        clustering[cluster_of[r]].append(r)
    return dict(name=name, ploidy=ploidy, n_pos=n_pos, error_rate=error_rate, reads=[[list(e) for e in row] for row in reads], haplotypes=haps,
                threads=threads, clustering=clustering, breakpoints=breakpoints)


def _read(rng, haps, h, start, stop, n_alleles, p_skip=0.15, p_err=0.08):
    row = []
    for p in range(start, stop):
        if rng.random() < p_skip:
            continue
        a = haps[h][p]
        if a < 0 or rng.random() < p_err:
            a = rng.randrange(n_alleles)
        row.append([p, a])
    return row or [[start, max(haps[h][start], 0)]]


def generic(name, seed, ploidy, n_pos, n_reads, n_alleles=2, n_clusters=None, mode="find", switch_rate=0.08, hom_rate=0.3, minus_rate=0.0,
            n_subsets=6, read_len=(3, 25), dup_reads=0, max_switch=2):
    rng = random.Random(seed)
    n_clusters = n_clusters or ploidy + 2
    haps = [[0] * n_pos for _ in range(ploidy)]
    for p in range(n_pos):
        col = [rng.randrange(n_alleles)] * ploidy if rng.random() < hom_rate else [rng.randrange(n_alleles) for _ in range(ploidy)]
        for h in range(ploidy):
            haps[h][p] = -1 if rng.random() < minus_rate else col[h]
    cur = [rng.randrange(n_clusters) for _ in range(ploidy)]
    threads = []
    for p in range(n_pos):
        if p and rng.random() < switch_rate:
            for h in rng.sample(range(ploidy), rng.randint(1, min(max_switch, ploidy))):
                cur[h] = rng.randrange(n_clusters)
        threads.append(list(cur))
    reads, cluster_of = [], []
    for _ in range(n_reads):
        h, start = rng.randrange(ploidy), rng.randrange(n_pos)
        row = _read(rng, haps, h, start, min(n_pos, start + rng.randint(*read_len)), n_alleles)
        reads.append(row)
        cluster_of.append(threads[row[len(row) // 2][0]][h])
    for r in rng.sample(range(n_reads), min(dup_reads, n_reads)):   # a position listed twice: the allele listed last counts
        x = rng.randrange(len(reads[r]))
        p, a = reads[r][x]
        reads[r].insert(x + 1, [p, (a + 1) % n_alleles])
    if mode == "find":
        breakpoints = find_breakpoints(threads)
    else:   # arbitrary sorted subsets at arbitrary positions (merged breakpoints exist)
        positions = sorted(rng.sample(range(1, n_pos), min(n_subsets, n_pos - 1)))
        breakpoints = [[p, sorted(rng.sample(range(ploidy), rng.randint(2, min(ploidy, 8))))] for p in positions]
    return _finish(name, rng, ploidy, n_pos, haps, threads, reads, cluster_of, n_clusters, breakpoints)


def window_limit():
    """More than 32 heterozygous positions on each side of the middle breakpoint; the outer windows are cut by the block's start and end.
    At positions 20 and 185 no haplotype switches: the clusters are the same on both sides."""
    rng = random.Random(101)
    n_pos = 200
    haps = [[0] * n_pos, [1] * n_pos]
    threads = [[0, 1] if p < 100 else [1, 0] for p in range(n_pos)]
    reads, cluster_of = [], []
    for _ in range(70):
        h, start = rng.randrange(2), rng.randrange(n_pos - 10)
        row = _read(rng, haps, h, start, min(n_pos, start + rng.randint(20, 90)), 2)
        reads.append(row)
        cluster_of.append(threads[row[0][0]][h])
    return _finish("window_limit", rng, 2, n_pos, haps, threads, reads, cluster_of, 2, [[20, [0, 1]], [100, [0, 1]], [185, [0, 1]]])


def empty_right_quirk():
    """From position 15 on the affected haplotypes 0 and 1 agree: right_pos is empty and the last window position is 14.  Read 0 starts
    exactly there, has an allele there and spans the breakpoint -- extractSubMatrix(.., removeEmpty = True) still drops it."""
    rng = random.Random(102)
    n_pos = 30
    haps = [[p % 2 for p in range(n_pos)], [(p + 1) % 2 if p < 15 else p % 2 for p in range(n_pos)], [rng.randrange(2) for _ in range(n_pos)]]
    threads = [[0, 0, 1] if p < 15 else [2, 3, 1] for p in range(n_pos)]
    reads = [[[p, haps[0][p]] for p in range(14, 21)], [[p, haps[1][p]] for p in range(14, 19)]]
    cluster_of = [0, 0]
    for _ in range(30):
        h, start = rng.randrange(3), rng.randrange(0, 14)
        reads.append(_read(rng, haps, h, start, min(n_pos, start + rng.randint(4, 20)), 2))
        cluster_of.append(threads[start][h])
    return _finish("empty_right_quirk", rng, 3, n_pos, haps, threads, reads, cluster_of, 4, [[15, [0, 1]]])


def duplicate_haplotypes():
    """Haplotypes 0 and 1 are equal everywhere.  Affected [0, 1]: both windows are empty, every permutation scores 0.0.  Affected
    [0, 1, 2]: the windows are not empty and the permutations that only exchange 0 and 1 tie by construction, twice."""
    rng = random.Random(103)
    n_pos = 40
    h0 = [rng.randrange(2) for _ in range(n_pos)]
    haps = [h0, list(h0), [1 - a if rng.random() < 0.7 else a for a in h0]]
    threads = [[0, 0, 1] if p < 12 else ([2, 0, 1] if p < 24 else [2, 3, 0]) for p in range(n_pos)]
    reads, cluster_of = [], []
    for _ in range(60):
        h, start = rng.randrange(3), rng.randrange(n_pos - 3)
        reads.append(_read(rng, haps, h, start, min(n_pos, start + rng.randint(4, 22)), 2))
        cluster_of.append(threads[start][h])
    return _finish("duplicate_haplotypes", rng, 3, n_pos, haps, threads, reads, cluster_of, 4, [[8, [0, 1]], [12, [0, 1, 2]], [24, [0, 1, 2]]])


def span_edges():
    """Breakpoint 10: reads end at 9 or start at 10, none spans it.  Breakpoint 25: spanning reads beside reads that end at 24 or start at 25."""
    rng = random.Random(104)
    n_pos = 40
    haps = [[rng.randrange(2) for _ in range(n_pos)] for _ in range(2)]
    for p in range(n_pos):
        haps[1][p] = 1 - haps[0][p] if p % 3 else haps[0][p]
    threads = [[0, 1] if p < 10 else ([1, 0] if p < 25 else [0, 2]) for p in range(n_pos)]
    spans = [(2, 10), (4, 10), (10, 18), (10, 14), (11, 20), (12, 25), (15, 25), (25, 33), (25, 40), (18, 31), (20, 28), (22, 36), (24, 26), (13, 38)]
    reads, cluster_of = [], []
    for a, b in spans * 2:
        h = rng.randrange(2)
        reads.append(_read(rng, haps, h, a, b, 2, p_skip=0.0))
        cluster_of.append(threads[a][h])
    return _finish("span_edges", rng, 2, n_pos, haps, threads, reads, cluster_of, 3, [[10, [0, 1]], [25, [0, 1]]])


def lds_tile():
    """One breakpoint with more spanning reads than one LDS tile of the permutation kernel holds."""
    rng = random.Random(105)
    n_pos, n = 40, read_tile() + 37
    haps = [[rng.randrange(3) for _ in range(n_pos)] for _ in range(3)]
    threads = [[0, 1, 2] if p < 20 else [1, 2, 0] for p in range(n_pos)]
    reads, cluster_of = [], []
    for _ in range(n):
        h, start = rng.randrange(3), rng.randrange(0, 19)
        reads.append(_read(rng, haps, h, start, rng.randint(22, n_pos), 3))
        cluster_of.append(threads[start][h])
    return _finish("lds_tile", rng, 3, n_pos, haps, threads, reads, cluster_of, 3, [[20, [0, 1, 2]]])


def seven_of_eight():
    """Seven affected haplotypes at ploidy 8: 5 040 permutations, twenty workgroups for one breakpoint."""
    c = generic("seven_of_eight", 106, 8, 50, 70, n_alleles=3, mode="subsets", n_subsets=1, hom_rate=0.1)
    c["breakpoints"] = [[26, [0, 1, 2, 3, 5, 6, 7]]]
    return c


def all_cases():
    cases = []
    seed = 1
    for ploidy in (2, 3, 4, 6):
        for mode in ("find", "subsets"):
            for _ in range(2):
                rng = random.Random(1000 + seed)
                cases.append(generic(f"random_p{ploidy}_{mode}_{seed}", seed, ploidy, rng.randint(30, 60), rng.randint(40, 80), n_alleles=rng.choice((2, 3)),
                                     mode=mode, switch_rate=0.12, max_switch=min(3, ploidy)))
                seed += 1
    cases.append(generic("alleles_0_to_3_and_minus_one", 50, 4, 50, 70, n_alleles=4, minus_rate=0.12, mode="subsets"))
    cases.append(generic("duplicate_positions", 51, 3, 40, 60, n_alleles=3, dup_reads=25, switch_rate=0.15))
    cases.append(generic("zero_breakpoints", 52, 3, 30, 40, switch_rate=0.0))
    cases += [window_limit(), empty_right_quirk(), duplicate_haplotypes(), span_edges(), lds_tile(), seven_of_eight()]
    assert not cases[-7]["breakpoints"]
    return cases


def medium_case():
    """Ploidy 6, about 300 positions and 600 reads (device against host twin; not recorded)."""
    return generic("medium", 77, 6, 300, 600, n_alleles=3, switch_rate=0.1, max_switch=3, read_len=(5, 60))


def large_problem(n_pos=20000, seed=5):
    """The benchmark's block (scripts/gpu_reorder_bench.py, profiles/reorder): hexaploid, three reads per position."""
    return generic("large", seed, 6, n_pos, 3 * n_pos, n_alleles=2, n_clusters=10, switch_rate=0.08, max_switch=6, read_len=(10, 80))


def load_golden():
    import gzip
    import json

    with gzip.open(os.path.join(ROOT, "tests", "golden", "reorder_cases.json.gz"), "rt") as f:
        return json.load(f)


def recorded_clusters(case):
    return [e["clusters"] for e in case["expected"]]


def check_against_recording(case, res):
    """One problem's result (whatshap_amd.reorder.ReorderResult, computed with the recorded cluster order) against what the reference
    recorded: every llh bit for bit, windows, chosen permutations, assignments, threads and haplotypes equal; a confidence within
    (4 + k!) * 2^-52 relative -- 2 ulp on the numerator's exp, 2 on the denominator's terms, at most one per add of the k! - 1 sequential
    adds (the libm that recorded need not be this machine's, hence a bound and not bits)."""
    import math

    import numpy as np

    exp = case["expected"]
    assert len(res.llh) == len(exp) == len(res.best) == len(res.confidence)
    for b, e in enumerate(exp):
        want = np.array([float.fromhex(v) for v in e["llh"]], dtype=np.float64)
        got = np.ascontiguousarray(res.llh[b], dtype=np.float64)
        assert got.view(np.uint64).tolist() == want.view(np.uint64).tolist(), (case["name"], b)
        assert res.windows[b] == (e["left"], e["right"]), (case["name"], b)
        assert int(res.best[b]) == e["chosen"], (case["name"], b)
        k = len(case["breakpoints"][b][1])
        conf = float.fromhex(case["confidence"][b])
        assert abs(float(res.confidence[b]) - conf) <= (4 + math.factorial(k)) * 2.0 ** -52 * abs(conf), (case["name"], b, float(res.confidence[b]), conf)
    assert res.assignments.tolist() == case["assignments"], case["name"]
    assert res.threads.tolist() == case["final_threads"], case["name"]
    assert res.haplotypes.tolist() == case["final_haplotypes"], case["name"]


def cluster_order(case):
    """Per breakpoint the clusters in the order this interpreter iterates the reference's set expression (what whatshap_amd.reorder's
    reference-signature functions pass on)."""
    out = []
    threads = case["threads"]
    for pos, affected in case["breakpoints"]:
        s = {threads[pos][h] for h in affected}
        if pos > 0:
            s = s.union({threads[pos - 1][h] for h in affected})
        out.append(list(s))
    return out


def allele_matrix(case):
    from whatshap_amd.polyphase import AlleleMatrix

    read_ptr, pos, alle = [0], [], []
    for row in case["reads"]:
        for p, a in row:
            pos.append(global_position(p))
            alle.append(a)
        read_ptr.append(len(pos))
    return AlleleMatrix.from_csr(read_ptr, pos, alle)


def problem(case, clusters=None):
    """The array-level problem of a case; ``clusters``: per breakpoint the ordered cluster list (default: cluster_order)."""
    from whatshap_amd.reorder import ReorderProblem

    bps = case["breakpoints"]
    return ReorderProblem(allele_matrix(case), case["threads"], case["haplotypes"], case["clustering"], [b[0] for b in bps], [b[1] for b in bps],
                          clusters if clusters is not None else cluster_order(case))
