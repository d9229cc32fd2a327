"""Seeded cases for the polyphase threading inputs (whatshap_amd/polythread.py): the smallest shapes at which each piece of
get_allele_depths, select_clusters and compute_haplotypes can go wrong, a few dozen random blocks, and the larger shapes that are only
compared between the device and the host twin.  tests/golden/make_polythread_golden.py records what the reference returns for
``all_cases()`` and ``select_cases()``; the tests read the recorded data.

A case: ``reads`` (rows of (local position, allele), as listed), ``n_pos``, ``clustering`` (lists of read ids, each in its own order),
``ploidy``, ``max_gap``.  A select case: ``depths`` per position as [[cluster, [[allele, count], ...]], ...] in dict order."""
import random

import numpy as np


def global_position(p):
    return 100 + 7 * p


def case(name, reads, clustering, ploidy, max_gap=10):
    n_pos = 1 + max(p for row in reads for p, _ in row)
    assert {p for row in reads for p, _ in row} == set(range(n_pos)), name
    return dict(name=name, reads=[[[int(p), int(a)] for p, a in row] for row in reads], n_pos=n_pos, clustering=[[int(r) for r in c] for c in clustering],
                ploidy=int(ploidy), max_gap=int(max_gap))


def from_depths(name, table, ploidy, max_gap=10, reverse=()):
    """One read per counted entry: table[pos] = {cluster: depth | [depth of allele 0, of allele 1, ...]}.  The reads of a cluster are listed
    in the order made (position by position, allele by allele); the clusters in ``reverse`` list theirs backwards."""
    reads, members = [], {}
    for pos, row in enumerate(table):
        for cid, depth in row.items():
            for allele, n in enumerate(depth if isinstance(depth, (list, tuple)) else [depth]):
                for _ in range(n):
                    members.setdefault(cid, []).append(len(reads))
                    reads.append([(pos, allele)])
    clustering = [members.get(c, []) for c in range(1 + max(members))]
    for c in reverse:
        clustering[c].reverse()
    return case(name, reads, clustering, ploidy, max_gap)


def hand_made():
    out = []
    # n_pos 1, 2, 3: the gap filling touches 1 .. n-2 only
    out.append(from_depths("one_position", [{0: 3, 1: 2}], 2))
    out.append(from_depths("two_positions", [{0: 3, 1: 2}, {1: 4}], 2))
    out.append(from_depths("three_positions_gap_in_the_middle", [{0: 3, 1: 2}, {0: 4}, {0: 2, 1: 2}], 2))
    out.append(case("one_read_one_cluster", [[(0, 1), (1, 0), (2, 1)]], [[0]], 2))
    out.append(case("cluster_with_an_empty_read", [[(0, 0), (1, 1)], [], [(1, 0)]], [[1, 0], [2]], 2))
    out.append(case("read_in_no_cluster", [[(0, 0), (1, 1)], [(0, 1), (1, 1)], [(0, 1)]], [[0], [2]], 2))
    out.append(case("position_listed_twice_in_a_read", [[(0, 0), (1, 1), (0, 1)], [(0, 0), (1, 0)]], [[0, 1]], 2))
    # consensus: ties by list order, the list not ascending in read id
    out.append(case("consensus_tie_list_descending", [[(0, 0)], [(0, 1)]], [[1, 0]], 3))
    out.append(case("consensus_tie_list_ascending", [[(0, 0)], [(0, 1)]], [[0, 1]], 3))
    out.append(case("consensus_two_halves_against_one", [[(0, 1)], [(0, 0)], [(0, 0)]], [[0, 1, 2]], 3))
    out.append(case("consensus_two_halves_against_one_other_order", [[(0, 1)], [(0, 0)], [(0, 0)]], [[2, 0, 1]], 3))
    out.append(from_depths("more_picks_than_alleles", [{0: [0, 0, 5]}], 6))
    out.append(from_depths("four_alleles", [{0: [3, 1, 4, 2], 1: [0, 2, 0, 2]}, {0: [1, 1, 1, 1], 1: [0, 0, 0, 6]}], 4, reverse=(0,)))
    # selection
    out.append(from_depths("more_clusters_than_slots", [{c: 5 + c % 3 for c in range(7)}, {c: 4 for c in range(6)}], 2))
    out.append(from_depths("equal_depths_across_the_cut", [{c: 2 for c in range(5)}], 1))
    for ploidy in (2, 3, 6):
        edge = 8 * ploidy - 1
        out.append(from_depths(f"threshold_exact_kept_ploidy{ploidy}", [{0: edge, 1: 1}], ploidy))
        out.append(from_depths(f"threshold_exact_dropped_ploidy{ploidy}", [{0: edge + 1, 1: 1}], ploidy))
    out.append(from_depths("low_cluster_ends_the_list", [{0: 40, 1: 1, 2: 1, 3: 10}], 2))
    out.append(from_depths("ploidy_one", [{0: 9, 1: 2}, {0: 1, 1: 7}, {1: 3}], 1))
    # gaps
    for max_gap in (0, 1, 2):
        gap = [{0: 5, 1: 5, 2: 5}] + [{0: 5}] * max_gap + [{0: 5, 1: 5}, {0: 5, 2: 5}, {0: 5}]   # cluster 1 is away for max_gap positions, cluster 2 for one more
        out.append(from_depths(f"gap_of_max_gap_{max_gap}_and_one_more", gap, 2, max_gap))
    out.append(from_depths("gap_reaching_the_last_position", [{0: 4, 1: 4}, {0: 4}, {0: 4}, {0: 4, 1: 4}], 2, 2))
    out.append(from_depths("gap_behind_the_last_position_is_not_looked_at", [{0: 4, 1: 4}, {0: 4}, {0: 4}], 2, 5))
    out.append(from_depths("capacity_full_breaks_the_chain", [{0: 5, 9: 5}, {0: 5}, {1: 5, 2: 5, 3: 5}, {0: 5}, {0: 5, 9: 5}], 1, 5))
    out.append(from_depths("two_candidates_one_slot", [{0: 5, 7: 9, 8: 7}, {0: 5, 1: 5}, {0: 5, 7: 5, 8: 5}], 1, 3))
    out.append(from_depths("two_candidates_one_slot_order_of_appending", [{0: 9, 7: 9, 8: 9}, {0: 5, 8: 5}, {0: 5, 1: 5}, {0: 5, 7: 5, 8: 5}], 1, 3))
    out.append(from_depths("readded_row_is_emptied", [{0: 20, 1: 20}, {0: [30, 10], 1: [0, 1]}, {0: 20, 1: 20}], 2, 1))
    out.append(from_depths("readded_without_a_row_next_to_an_emptied_one", [{0: 30, 1: 30, 2: 30}, {0: 60, 1: [1, 0]}, {0: 30, 1: 30, 2: 30}], 2, 1))
    out.append(from_depths("did_not_fit_cannot_be_carried_on", [{0: 9, 5: 8, 6: 7}, {0: 5, 1: 5, 2: 5}, {0: 5}, {0: 5, 5: 5, 6: 5}], 1, 4))
    return out


def random_case(seed, n_pos, n_reads, ploidy, n_alleles, max_gap, read_len, n_clusters=None, unclustered=0.05, shuffle=True):
    """Reads as windows of one of `ploidy` random haplotypes with noise, clustered by haplotype and stretch of the block (so clusters come
    and go along the block), some reads left out of every cluster; every position is covered by a clustered read."""
    rng = random.Random(seed)
    haps = [[rng.randrange(n_alleles) for _ in range(n_pos)] for _ in range(ploidy)]
    stretch = max(2, n_pos // 3)
    reads, key_of = [], []
    for _ in range(n_reads):
        h = rng.randrange(ploidy)
        start = rng.randrange(n_pos)
        length = rng.randint(1, read_len)
        row = []
        for p in range(start, min(n_pos, start + length)):
            if rng.random() < 0.15:
                continue
            a = haps[h][p] if rng.random() > 0.1 else rng.randrange(n_alleles)
            row.append((p, a))
        reads.append(row)
        key_of.append((h, start // stretch) if rng.random() > 0.08 else (rng.randrange(ploidy), start // stretch))
    covered = set()
    keys = sorted(set(key_of))
    if n_clusters:
        keys = keys[:n_clusters]
    clustering = [[] for _ in keys]
    for r, k in enumerate(key_of):
        if k in keys and reads[r] and rng.random() >= unclustered:
            clustering[keys.index(k)].append(r)
            covered |= {p for p, _ in reads[r]}
    for p in range(n_pos):
        if p not in covered:
            clustering[rng.randrange(len(clustering))].append(len(reads))
            reads.append([(p, haps[0][p])])
    if shuffle:
        for c in clustering:
            rng.shuffle(c)
    return case(f"random_seed{seed}_p{ploidy}_a{n_alleles}_g{max_gap}", reads, clustering, ploidy, max_gap)


def random_cases():
    out = []
    seed = 100
    for ploidy, n_alleles in ((1, 2), (2, 2), (3, 2), (4, 3), (6, 4), (2, 4), (3, 3), (4, 2), (6, 2)):
        for max_gap, n_pos, n_reads, read_len in ((2, 40, 80, 8), (10, 150, 260, 12)):
            out.append(random_case(seed, n_pos, n_reads, ploidy, n_alleles, max_gap, read_len))
            seed += 1
    out.append(random_case(seed, 60, 400, 2, 2, 3, 10, n_clusters=9))
    out.append(random_case(seed + 1, 30, 300, 1, 3, 1, 6))
    return out


def all_cases():
    return hand_made() + random_cases()


def uncovered_case():
    """A position only a read outside every cluster covers: the reference's select_clusters raises IndexError."""
    return case("position_without_a_counted_entry", [[(0, 0), (1, 1)], [(1, 0), (2, 1)], [(3, 0)]], [[0], [2]], 2)


def select_cases():
    """select_clusters on dicts as a caller may hand them: clusters not in ascending order, equal depths, empty inner dicts."""
    def pos(*rows):
        return [[cid, [[a, n] for a, n in alleles]] for cid, alleles in rows]

    return [
        dict(name="dict_order_decides_equal_depths", ploidy=1, max_gap=2,
             depths=[pos((5, [(0, 2)]), (3, [(1, 2)]), (9, [(0, 1), (1, 1)]), (1, [(0, 2)])), pos((3, [(0, 4)])), pos((1, [(0, 3)]), (5, [(0, 3)]))]),
        dict(name="empty_inner_dict_and_large_ids", ploidy=2, max_gap=1,
             depths=[pos((70000, [(0, 6)]), (4, [])), pos((4, [(1, 3)])), pos((4, [(1, 3)]), (70000, [(0, 5), (2, 1)]))]),
        dict(name="emptied_in_place_keeps_the_dict_order", ploidy=2, max_gap=3,
             depths=[pos((2, [(0, 20)]), (1, [(0, 20)])), pos((1, [(0, 1)]), (2, [(0, 40)]), (0, [(1, 1)])), pos((0, [(0, 9)])), pos((1, [(0, 20)]), (2, [(0, 20)]))]),
    ]


# ---------------------------------------------------------------------------------------------- larger shapes: device against host twin only
def csr_of(c):
    """(read_ptr, global positions, alleles) of a case's reads."""
    read_ptr = np.zeros(len(c["reads"]) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in c["reads"]], out=read_ptr[1:])
    flat = [e for r in c["reads"] for e in r]
    pos = np.asarray([global_position(p) for p, _ in flat], dtype=np.int64)
    alle = np.asarray([a for _, a in flat], dtype=np.int64)
    return read_ptr, pos, alle


def array_problem(seed, n_pos, coverage, ploidy, n_alleles, read_len, n_stretches, max_gap=10, unclustered=0.02):
    """A block as arrays (numpy throughout, any size): reads of ``read_len`` consecutive positions drawn from ``ploidy`` haplotypes,
    clusters = haplotype x stretch of the block with a few reads moved to another haplotype's cluster, cluster lists shuffled.
    Returns (read_ptr, positions, alleles, clustering as a list of arrays)."""
    rng = np.random.default_rng(seed)
    n_reads = max(1, n_pos * coverage // read_len)
    haps = rng.integers(0, n_alleles, size=(ploidy, n_pos), dtype=np.int64)
    start = np.sort(rng.integers(0, max(1, n_pos - read_len + 1), size=n_reads))
    start[0] = 0
    length = np.minimum(read_len, n_pos - start)
    # every position covered: chain the starts so that no gap is left
    for r in range(1, n_reads):
        if start[r] > start[r - 1] + length[r - 1]:
            start[r] = start[r - 1] + length[r - 1]
    length = np.minimum(read_len, n_pos - start)
    if start[-1] + length[-1] < n_pos:
        start[-1] = n_pos - length[-1]
    hap = rng.integers(0, ploidy, size=n_reads)
    read_ptr = np.zeros(n_reads + 1, dtype=np.uint64)
    np.cumsum(length, out=read_ptr[1:])
    read_of = np.repeat(np.arange(n_reads), length)
    local = np.arange(int(read_ptr[-1])) - np.repeat(read_ptr[:-1].astype(np.int64), length) + start[read_of]
    alle = haps[hap[read_of], local]
    noise = rng.random(alle.size) < 0.08
    alle = np.where(noise, rng.integers(0, n_alleles, size=alle.size), alle)
    stretch = np.minimum(start * n_stretches // max(1, n_pos), n_stretches - 1)
    moved = rng.random(n_reads) < 0.05
    cl = np.where(moved, rng.integers(0, ploidy, size=n_reads), hap) * n_stretches + stretch
    out_of_all = rng.random(n_reads) < unclustered
    out_of_all[0] = False
    # a read left out must not uncover a position: keep it in if it is the only cover of one
    cover = np.zeros(n_pos + 1, dtype=np.int64)
    keep = ~out_of_all
    np.add.at(cover, start[keep], 1)
    np.add.at(cover, start[keep] + length[keep], -1)
    bare = np.flatnonzero(np.cumsum(cover)[:n_pos] == 0)
    for p in bare.tolist():
        r = int(np.searchsorted(start, p, side="right")) - 1
        out_of_all[r] = False
    clustering = []
    for c in range(ploidy * n_stretches):
        members = np.flatnonzero((cl == c) & ~out_of_all).astype(np.uint32)
        rng.shuffle(members)
        clustering.append(members)
    return read_ptr, 100 + 7 * local, alle, clustering


BENCH = dict(ploidy=6, n_alleles=2, read_len=30, max_gap=10)


def bench_arrays(n_pos=500_000, coverage=40):
    """The benchmark's chromosome: hexaploid, reads of 30 consecutive positions, clusters of about 2 000 positions per haplotype."""
    return array_problem(11, n_pos, coverage, BENCH["ploidy"], BENCH["n_alleles"], BENCH["read_len"], max(1, n_pos // 2000), BENCH["max_gap"])


def prefix_of(arrays, n_pos):
    """The first n_pos positions of a block made by array_problem: every read cut there, reads left empty dropped, read ids renumbered."""
    read_ptr, pos, alle, clustering = arrays
    keep_entry = pos < 100 + 7 * n_pos
    read_of = np.repeat(np.arange(len(read_ptr) - 1), np.diff(read_ptr.astype(np.int64)))
    lengths = np.bincount(read_of[keep_entry], minlength=len(read_ptr) - 1)
    kept = np.flatnonzero(lengths > 0)
    new_id = np.full(len(read_ptr) - 1, -1, dtype=np.int64)
    new_id[kept] = np.arange(kept.size)
    new_ptr = np.zeros(kept.size + 1, dtype=np.uint64)
    np.cumsum(lengths[kept], out=new_ptr[1:])
    new_clustering = [new_id[c][new_id[c] >= 0].astype(np.uint32) for c in clustering]
    return new_ptr, pos[keep_entry], alle[keep_entry], [c for c in new_clustering if c.size]


def small_blocks(n, seed=500):
    """n small blocks of different ploidies, allele counts and gaps: (arrays, ploidy, max_gap) each."""
    out = []
    for k in range(n):
        ploidy = (2, 3, 4, 6, 1)[k % 5]
        out.append((array_problem(seed + k, 20 + 7 * (k % 9), 10 + k % 7, ploidy, 2 + k % 3, 4 + k % 5, 1 + k % 3, unclustered=0.05), ploidy, k % 4))
    return out


def long_run_case():
    """One position with a run of several thousand entries over a handful of clusters, one of a few hundred, next to positions of one
    entry: every run class."""
    rng = np.random.default_rng(7)
    n_pos = 12
    reads, cluster_of = [], []
    for _ in range(6000):
        reads.append([(5, int(rng.integers(0, 3)))])
        cluster_of.append(int(rng.integers(0, 5)))
    for _ in range(300):
        reads.append([(8, int(rng.integers(0, 3))), (9, int(rng.integers(0, 3)))])
        cluster_of.append(int(rng.integers(0, 7)))
    for p in range(n_pos):
        reads.append([(p, int(rng.integers(0, 3)))])
        cluster_of.append(int(rng.integers(0, 7)))
    clustering = [[] for _ in range(7)]
    for r in rng.permutation(len(reads)).tolist():
        clustering[cluster_of[r]].append(r)
    return case("long_run", reads, clustering, 3, 4)


def sixteen_allele_long_runs_case(deep=4200, wide=300):
    """Ploidy 16, all sixteen alleles: one position of ``deep`` entries (one workgroup: more than PT_CLASS_B_MAX = 4096), one of ``wide``
    (one wave), each over four clusters and every allele, next to positions of one entry."""
    rng = np.random.default_rng(16)

    def spread(total, clusters):
        """total entries over the clusters and the sixteen alleles, every (cluster, allele) at least once."""
        cells = rng.multinomial(total - 16 * len(clusters), np.full(16 * len(clusters), 1.0 / (16 * len(clusters)))) + 1
        return {c: cells[16 * k:16 * k + 16].tolist() for k, c in enumerate(clusters)}

    one = lambda c, allele: {c: [0] * allele + [1]}
    table = [one(0, 3), spread(wide, (0, 2, 3, 5)), one(4, 15), one(1, 0), spread(deep, (1, 2, 4, 5)), one(5, 9), one(3, 7)]
    return from_depths("sixteen_alleles_long_runs", table, 16, 2, reverse=(2, 5))


# The reads around a workgroup's edge (256 entries per workgroup in the count and place launches): entries 255 and 256 are single-entry
# reads with empty reads before, between and behind.
EDGE_READ_LENGTHS = (0, 255, 0, 0, 1, 1, 0, 343, 0)


def edge_read_ptr(n_entries=600):
    """EDGE_READ_LENGTHS as offsets, the reads cut at ``n_entries`` (the reads behind the cut stay, empty)."""
    ptr = np.minimum(np.concatenate([[0], np.cumsum(EDGE_READ_LENGTHS)]), n_entries)
    assert ptr[-1] == n_entries
    return ptr.astype(np.uint64)


def edge_reads_arrays(n_entries=600, n_clusters=5):
    """A block on the reads of edge_read_ptr: a read's k-th entry lies at position k (the matrix keeps one entry per read and position,
    so a read of 343 entries needs as many positions), a single-entry read's in the middle of the block; the alleles are random, every
    read -- the empty ones too -- is in one of ``n_clusters`` clusters."""
    rng = np.random.default_rng(600 + n_entries)
    read_ptr = edge_read_ptr(n_entries)
    lengths = np.diff(read_ptr.astype(np.int64))
    local = np.arange(n_entries) - np.repeat(read_ptr[:-1].astype(np.int64), lengths)
    single = np.flatnonzero(np.repeat(lengths, lengths) == 1)
    if n_entries > 1:
        local[single] = 100 + 50 * np.arange(single.size)
    alle = rng.integers(0, 2, size=n_entries)
    cluster_of = rng.integers(0, n_clusters, size=len(read_ptr) - 1)
    clustering = [rng.permutation(np.flatnonzero(cluster_of == c)).astype(np.uint32) for c in range(n_clusters)]
    return read_ptr, 100 + 7 * local, alle, clustering


# ---------------------------------------------------------------------------------------------- what both test files share
def load_golden():
    import gzip
    import json
    import os

    with gzip.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "polythread_cases.json.gz")) as f:
        return json.load(f)


def matrix_of(c):
    from whatshap_amd.polyphase import AlleleMatrix

    return AlleleMatrix.from_csr(*csr_of(c))


def problem_of(c, **kw):
    from whatshap_amd.polythread import ThreadingProblem

    return ThreadingProblem(matrix_of(c), c["clustering"], c["ploidy"], c["max_gap"], **kw)


def problem_of_arrays(arrays, ploidy, max_gap):
    from whatshap_amd.polyphase import AlleleMatrix
    from whatshap_amd.polythread import ThreadingProblem

    read_ptr, pos, alle, clustering = arrays
    return ThreadingProblem(AlleleMatrix.from_csr(read_ptr, pos, alle), clustering, ploidy, max_gap)


def as_pairs(dicts):
    """Dict forms as the golden file holds them: lists of pairs in dict order."""
    return [[[cid, [[a, n] for a, n in v.items()] if isinstance(v, dict) else list(v)] for cid, v in d.items()] for d in dicts]


def as_dicts(pair_lists):
    return [{cid: {a: n for a, n in v} for cid, v in position} for position in pair_lists]


def check_against_record(res, rec):
    """One problem's arrays and dict forms against everything the reference recorded for the case."""
    n_alleles = res.n_alleles
    ad, cons = res._dicts()
    assert as_pairs(ad) == rec["ad_after"], rec["name"]
    assert as_pairs(cons) == rec["cons_lists"], rec["name"]
    assert res.cov_map() == rec["cov_map"], rec["name"]
    # the arrays, from the record: rows ascending in the cluster, depths after the side effect, first in insertion order
    ptr, cluster, depth, cons_rows, order = [0], [], [], [], []
    for before, after, lists in zip(rec["ad"], rec["ad_after"], rec["cons_lists"]):
        after, lists = dict((cid, v) for cid, v in after), dict((cid, v) for cid, v in lists)
        for cid, alleles in sorted(before):
            row = [0] * n_alleles
            for a, n in after[cid]:
                row[a] = n
            cluster.append(cid)
            depth.append(row)
            cons_rows.append(lists[cid])
            order.append([a for a, _ in alleles])
        ptr.append(len(cluster))
    assert res.pc_ptr.tolist() == ptr and res.pc_cluster.tolist() == cluster, rec["name"]
    assert res.pc_depth.tolist() == depth and res.pc_consensus.tolist() == cons_rows, rec["name"]
    none = 0xFFFFFFFF
    for row, alleles in zip(res.pc_first.tolist(), order):
        assert sorted((a for a in range(n_alleles) if row[a] != none), key=lambda a: row[a]) == alleles, rec["name"]
    cov_ptr = np.cumsum([0] + [len(x) for x in rec["cov_map"]]).tolist()
    assert res.cov_ptr.tolist() == cov_ptr and res.cov_cluster.tolist() == [c for x in rec["cov_map"] for c in x], rec["name"]
    # re-added: in the list, but not among what the position's own depths select -- the reference's dicts show it as an emptied or a new row
    for x, (before, after) in enumerate(zip(rec["ad"], rec["ad_after"])):
        before = dict((cid, v) for cid, v in before)
        changed = {cid for cid, v in after if before.get(cid) != v}
        b, e = int(res.cov_ptr[x]), int(res.cov_ptr[x + 1])
        got = {int(c) for c, r in zip(res.cov_cluster[b:e], res.cov_readded[b:e]) if r}
        assert changed <= got and all(not dict((c, v) for c, v in after)[cid] for cid in got), rec["name"]
        assert sorted(res.cov_rank[b:e].tolist()) == list(range(e - b)), rec["name"]
