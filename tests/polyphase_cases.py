"""Recorded polyphase read-scoring cases (tests/golden/polyphase_cases.json.gz, tests/golden/make_polyphase_golden.py) as CSR arrays
and AlleleMatrix objects, and a generator of larger random blocks shaped like long-read polyploid data."""
import gzip
import json
import os

import numpy as np

from whatshap_amd.polyphase import AlleleMatrix

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "polyphase_cases.json.gz")


def load():
    with gzip.open(GOLDEN, "rt") as f:
        return json.load(f)["cases"]


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
