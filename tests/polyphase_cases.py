"""Recorded polyphase read-scoring cases (tests/golden/polyphase_cases.json.gz and polyphase_edge_cases.json.gz, both written by
tests/golden/make_polyphase_golden.py) as CSR arrays and AlleleMatrix objects, and a generator of larger random blocks shaped like
long-read polyploid data."""
import gzip
import json
import os

import numpy as np

from whatshap_amd.polyphase import AlleleMatrix

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "polyphase_cases.json.gz")


GOLDEN_EDGE = os.path.join(os.path.dirname(GOLDEN), "polyphase_edge_cases.json.gz")
EDGE_KINDS = ("nan", "high_ploidy", "many_alleles", "sparse_positions", "long_overlap")
BITMAP_SLACK = 1 << 20   # poly_build_matrix (csrc/polyscore.cpp): a bitmap of the span while span <= 64 * n_entries + 2^20, else a sort


def load():
    with gzip.open(GOLDEN, "rt") as f:
        return json.load(f)["cases"]


def load_edge():
    """The second recording: the kinds of EDGE_KINDS.  Every sparse_positions case lies on the side of poly_build_matrix's threshold
    that its place in the file promises (the last but one exactly at it, the others above)."""
    with gzip.open(GOLDEN_EDGE, "rt") as f:
        cases = json.load(f)["cases"]
    assert {c["kind"] for c in cases} == set(EDGE_KINDS)
    sparse = [c for c in cases if c["kind"] == "sparse_positions"]
    for c in sparse:
        span, n_entries = span_and_entries(c)
        assert span == 64 * n_entries + BITMAP_SLACK if c is sparse[-2] else takes_sort_branch(c)
    return cases


def span_and_entries(case):
    pos = [e[0] for r in case["reads"] for e in r]
    return (max(pos) - min(pos) + 1, len(pos)) if pos else (0, 0)


def takes_sort_branch(case) -> bool:
    """Whether poly_build_matrix sorts this case's positions (the inequality of its bitmap branch, negated)."""
    span, n_entries = span_and_entries(case)
    return n_entries > 0 and span > 64 * n_entries + BITMAP_SLACK


def matrix(case) -> AlleleMatrix:
    reads = case["reads"]
    read_ptr = np.zeros(len(reads) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in reads], out=read_ptr[1:])
    pos = np.array([e[0] for r in reads for e in r], dtype=np.int64)
    alle = np.array([e[1] for r in reads for e in r], dtype=np.int64)
    return AlleleMatrix.from_csr(read_ptr, pos, alle)


def expected(case):
    e = case["expected"]
    return (np.asarray(e["i"], dtype=np.uint32), np.asarray(e["j"], dtype=np.uint32),
            np.asarray(e["bits"], dtype=np.uint32).view(np.float32))


def ulp_distance(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """|a - b| in float32 ulps (same-sign finite values)."""
    ia = a.astype(np.float32).view(np.int32).astype(np.int64)
    ib = b.astype(np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def random_block(seed, n_reads, n_pos, ploidy=4, n_alleles=2, min_len=20, max_len=300, p_keep=0.9, p_err=0.05, long_every=0, long_len=0):
    """CSR arrays of a block drawn from `ploidy` haplotypes: reads of min_len .. max_len consecutive variants (sorted by position);
    every `long_every`-th read spans `long_len` variants (anchors far beyond any LDS budget)."""
    rng = np.random.default_rng(seed)
    haps = rng.integers(0, n_alleles, size=(ploidy, n_pos), dtype=np.int64)
    starts = np.sort(rng.integers(0, n_pos, size=n_reads))
    lens = rng.integers(min_len, max_len + 1, size=n_reads)
    if long_every:
        lens[::long_every] = long_len
    rows_p, rows_a, ptr = [], [], [0]
    for s, l in zip(starts, lens):
        p = np.arange(s, min(n_pos, s + l))
        p = p[rng.random(len(p)) < p_keep]
        if len(p) == 0:
            p = np.array([s])
        h = rng.integers(ploidy)
        a = haps[h, p].copy()
        flip = rng.random(len(p)) < p_err
        a[flip] = rng.integers(0, n_alleles, size=int(flip.sum()))
        rows_p.append(1000 + 13 * p)
        rows_a.append(a)
        ptr.append(ptr[-1] + len(p))
    return np.asarray(ptr, dtype=np.uint64), np.concatenate(rows_p).astype(np.int64), np.concatenate(rows_a).astype(np.int64)


def pair_count_matrix(stored):
    """A matrix with exactly len(stored) candidate pairs at minOverlap 2, two alleles: read 0 spans every position and read q (1, 2, ...)
    lists positions 2q and 2q + 1 only, so the pairs are (0, q) in anchor order and no two short reads are candidates of each other.
    Pair q shares both positions when stored[q - 1] (a score other than 0: one read shows allele 1 at 2q), else read 0 lacks 2q + 1 and
    the pair shares one position, too little.  Returns (matrix, n_pair_positions)."""
    n = len(stored)
    long_read = [0] + [p for q in range(1, n + 1) for p in ((2 * q, 2 * q + 1) if stored[q - 1] else (2 * q,))] + [2 * n + 2]
    pos, alle, ptr = list(long_read), [0] * len(long_read), [0, len(long_read)]
    for q in range(1, n + 1):
        pos += [2 * q, 2 * q + 1]
        alle += [1, 0]
        ptr.append(len(pos))
    return AlleleMatrix.from_csr(ptr, pos, alle), sum(2 if s else 1 for s in stored)
