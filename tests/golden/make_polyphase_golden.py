#!/usr/bin/env python3
"""Writes tests/golden/polyphase_cases.json.gz: what the reference's polyphase read scoring returns (run only where the reference tree
exists; the tests read the recorded data).

The reference's src/polyphase/{readscoring,allelematrix,trianglesparsematrix}.cpp and the src/*.cpp they need are compiled with a small
driver (written here, below) into a temporary directory outside the repository.  Per case the driver builds a ReadSet of Read objects,
AlleleMatrix(ReadSet*) on it, and records
  - the AlleleMatrix getters (positions, first / last position, depths, max allele) of matrices with at most 200 reads,
  - estimateAlleleErrorRate when err == 0 (what scoreReadset then uses),
  - scoreReadset: every stored entry (i > j, score as float bits) sorted by triangular index, and the NaN count of its warning.
Cases: several hundred seeded small matrices (ploidy 2, 3, 4, 6; 2 - 4 alleles; err 0, 0.07, 0.2; minOverlap 0, 1, 2, 5) drawn from
ploidy haplotypes with allele errors, plus single-position reads, duplicate positions, positions with one allele, depth >= 2000 at a
position (the halving path), ties in first position, disjoint reads, ploidy < 2, the empty matrix, and two matrices of 2 000 reads.
Usage: python tests/golden/make_polyphase_golden.py [/path/to/reference]

With --edge it writes tests/golden/polyphase_edge_cases.json.gz instead and leaves polyphase_cases.json.gz as it is: the same driver and
record format on the inputs the first recording lacks (edge_cases below) -- NaN scores, ploidy 7 - 15, up to 16 alleles, positions
spread so far apart that poly_build_matrix sorts them instead of marking a bitmap, and reads that share thousands of positions.
Usage: python tests/golden/make_polyphase_golden.py --edge [/path/to/reference]
"""
import gzip
import json
import os
import random
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "polyphase_cases.json.gz")
OUT_EDGE = os.path.join(HERE, "polyphase_edge_cases.json.gz")

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include <algorithm>
#include "readset.h"
#include "read.h"
#include "polyphase/allelematrix.h"
#include "polyphase/readscoring.h"
#include "polyphase/trianglesparsematrix.h"

int main(int argc, char** argv) {
    FILE* out = fopen(argv[1], "w");
    int n_cases;
    if (scanf("%d", &n_cases) != 1) return 1;
    for (int c = 0; c < n_cases; c++) {
        unsigned ploidy, min_overlap, n_reads, getters;
        char errs[64];
        if (scanf("%u %u %63s %u %u", &ploidy, &min_overlap, errs, &n_reads, &getters) != 5) return 1;
        double err = strtod(errs, nullptr);
        ReadSet* rs = new ReadSet();
        for (unsigned r = 0; r < n_reads; r++) {
            unsigned k;
            if (scanf("%u", &k) != 1) return 1;
            Read* read = new Read("r" + std::to_string(r), 60, 0, 0);
            for (unsigned x = 0; x < k; x++) {
                int p, a;
                if (scanf("%d %d", &p, &a) != 2) return 1;
                read->addVariant(p, a, 10);
            }
            rs->add(read);
        }
        AlleleMatrix am(rs);
        ReadScoring rsc;
        std::ostringstream captured;
        std::streambuf* saved = std::cout.rdbuf(captured.rdbuf());
        double used = err;
        if (err == 0.0 && ploidy >= 2) used = rsc.estimateAlleleErrorRate(&am, ploidy);
        std::ostringstream scored;
        std::cout.rdbuf(scored.rdbuf());
        TriangleSparseMatrix tsm;
        rsc.scoreReadset(&tsm, &am, min_overlap, ploidy, err);
        std::cout.rdbuf(saved);
        std::string s = scored.str();
        unsigned long nans = 0;
        size_t w = s.find("Warning: Found ");
        if (w != std::string::npos) nans = strtoul(s.c_str() + w + 15, nullptr, 10);
        std::vector<uint64_t> idx = tsm.getIndices();   // sorted triangular indices
        fprintf(out, "case %a %lu %zu\n", used, nans, idx.size());
        uint64_t u = 1;
        for (uint64_t t : idx) {
            while (u * (u + 1) / 2 <= t) u++;
            uint64_t v = t - u * (u - 1) / 2;
            float f = tsm.get((uint32_t)u, (uint32_t)v);
            uint32_t bits;
            memcpy(&bits, &f, 4);
            fprintf(out, "%lu %lu %u\n", (unsigned long)u, (unsigned long)v, bits);
        }
        if (getters) {
            fprintf(out, "positions");
            for (auto p : am.getPositions()) fprintf(out, " %u", p);
            fprintf(out, "\nfirst");
            for (uint32_t r = 0; r < am.size(); r++) fprintf(out, " %u", am.getFirstPos(r));
            fprintf(out, "\nlast");
            for (uint32_t r = 0; r < am.size(); r++) fprintf(out, " %u", am.getLastPos(r));
            fprintf(out, "\nmaxallele %d\ndepths", (int)am.getMaxNumAllele());
            for (uint32_t p = 0; p < am.getNumPositions(); p++)
                for (auto d : am.getAlleleDepths(p)) fprintf(out, " %u", d);
            fprintf(out, "\nrows");
            for (uint32_t r = 0; r < am.size(); r++) {
                auto row = am.getRead(r);
                fprintf(out, " %zu", row.size());
                for (auto& e : row) fprintf(out, " %u %d", e.first, (int)e.second);
            }
            fprintf(out, "\n");
        }
        delete rs;
    }
    fclose(out);
    return 0;
}
"""

SOURCES = ["read.cpp", "readset.cpp", "entry.cpp", "indexset.cpp", "genotype.cpp", "binomial.cpp", "multinomial.cpp",
           "polyphase/readscoring.cpp", "polyphase/allelematrix.cpp", "polyphase/trianglesparsematrix.cpp"]


def build_driver(ref_root, tmp):
    src = os.path.join(tmp, "driver.cpp")
    open(src, "w").write(DRIVER)
    exe = os.path.join(tmp, "poly_driver")
    srcdir = os.path.join(ref_root, "src")
    subprocess.run(["g++", "-O2", "-std=c++14", "-I" + srcdir, src] + [os.path.join(srcdir, s) for s in SOURCES] + ["-o", exe], check=True)
    return exe


# ---------------------------------------------------------------------------------------------- cases
def haplotype_reads(rng, n_reads, n_pos, ploidy, n_alleles, min_len, max_len, p_keep=0.85, p_err=0.05, spacing=7):
    haps = [[rng.randrange(n_alleles) for _ in range(n_pos)] for _ in range(ploidy)]
    reads = []
    for _ in range(n_reads):
        h = rng.randrange(ploidy)
        start = rng.randrange(n_pos)
        length = rng.randint(min_len, max_len)
        row = []
        for p in range(start, min(n_pos, start + length)):
            if rng.random() > p_keep:
                continue
            a = haps[h][p]
            if rng.random() < p_err:
                a = rng.randrange(n_alleles)
            row.append((100 + p * spacing, a))
        if not row:
            row.append((100 + start * spacing, haps[h][start]))
        reads.append(row)
    return reads


def small_cases(rng):
    cases = []
    combos = [(p, a, e, mo) for p in (2, 3, 4, 6) for a in (2, 3, 4) for e in (0.0, 0.07, 0.2) for mo in (0, 1, 2, 5)]
    for ploidy, n_alleles, err, mo in combos * 2:
        n_reads = rng.randint(2, 40)
        n_pos = rng.randint(1, 40)
        reads = haplotype_reads(rng, n_reads, n_pos, ploidy, n_alleles, 1, 15)
        cases.append(dict(kind="random", ploidy=ploidy, min_overlap=mo, err=err, reads=reads))
    return cases


def special_cases(rng):
    cases = []
    # single-position reads
    reads = [[(50 + 10 * rng.randrange(5), rng.randrange(2))] for _ in range(25)]
    for mo in (0, 1, 2):
        cases.append(dict(kind="single_position", ploidy=2, min_overlap=mo, err=0.07, reads=reads))
    # duplicate positions: a position listed twice keeps the last allele, both count in the depths
    for k in range(6):
        reads = haplotype_reads(rng, 20, 15, 3, 3, 2, 8)
        for r in reads[: 10]:
            p, a = r[rng.randrange(len(r))]
            r.append((p, (a + 1) % 3))
            r.sort(key=lambda e: e[0])   # sorted by position (stable: the added one stays last of its position)
        cases.append(dict(kind="duplicates", ploidy=3, min_overlap=k % 3, err=(0.0, 0.07)[k % 2], reads=reads))
    # positions with one allele only
    for ploidy in (2, 4):
        reads = haplotype_reads(rng, 30, 20, ploidy, 2, 3, 10, p_err=0.0)
        reads = [[(p, 0 if (p // 7) % 3 == 0 else a) for p, a in r] for r in reads]
        for err in (0.0, 0.07):
            cases.append(dict(kind="one_allele", ploidy=ploidy, min_overlap=1, err=err, reads=reads))
    # depth >= 2000 at some positions (the halving path): reads listing one position hundreds of times
    for n_alleles, ploidy in ((2, 2), (2, 4), (3, 3), (4, 6)):
        reads = haplotype_reads(rng, 20, 10, ploidy, n_alleles, 2, 6)
        hot = 100 + 3 * 7
        for t in range(5):
            a = t % n_alleles
            reads.append(sorted([(hot, a)] * 450 + [(hot + 7, (a + 1) % n_alleles)], key=lambda e: e[0]))
        for err in (0.0, 0.07):
            cases.append(dict(kind="deep", ploidy=ploidy, min_overlap=1, err=err, reads=reads))
    # ties in first position
    for mo in (1, 2, 5):
        reads = []
        for s in range(4):
            for _ in range(6):
                length = rng.randint(1, 12)
                reads.append([(100 + (s + x) * 5, rng.randrange(3)) for x in range(length)])
        rng.shuffle(reads)
        cases.append(dict(kind="ties", ploidy=3, min_overlap=mo, err=0.07, reads=reads))
    # disjoint reads
    reads = [[(100 + 20 * r + x, rng.randrange(2)) for x in range(3)] for r in range(12)]
    for mo in (0, 1):
        cases.append(dict(kind="disjoint", ploidy=2, min_overlap=mo, err=0.07, reads=reads))
    # ploidy < 2, the empty matrix
    reads = haplotype_reads(rng, 10, 8, 2, 2, 2, 5)
    for ploidy in (0, 1):
        cases.append(dict(kind="ploidy_below_2", ploidy=ploidy, min_overlap=1, err=0.07, reads=reads))
    for err in (0.0, 0.07):
        cases.append(dict(kind="empty", ploidy=4, min_overlap=1, err=err, reads=[]))
    return cases


def medium_cases(rng):
    cases = []
    for ploidy, n_alleles, err in ((4, 2, 0.07), (6, 3, 0.0)):
        reads = haplotype_reads(rng, 2000, 1500, ploidy, n_alleles, 3, 12, spacing=3)
        reads.sort(key=lambda r: r[0][0])
        cases.append(dict(kind="medium", ploidy=ploidy, min_overlap=2, err=err, reads=reads))
    return cases


# ---------------------------------------------------------------------------------------------- edge cases (--edge)
BITMAP_SLACK = 1 << 20   # poly_build_matrix (csrc/polyscore.cpp) marks a bitmap while span <= 64 * n_entries + 2^20, else it sorts


def indexed_reads(rng, n_reads, n_pos, ploidy, alleles_at, min_len, max_len, p_keep=0.9, p_err=0.05, max_start=None, n_long=0, long_len=0):
    """Reads as lists of (position index, allele) drawn from `ploidy` haplotypes; alleles_at[p] lists the alleles position p may show.
    The first read starts at index 0 and the last one ends at index n_pos - 1, so both ends of the index range are used; the first
    `n_long` reads list `long_len` indices instead of min_len .. max_len."""
    haps = [[rng.choice(alleles_at[p]) for p in range(n_pos)] for _ in range(ploidy)]
    reads = []
    for r in range(n_reads):
        h = rng.randrange(ploidy)
        length = long_len if r < n_long else rng.randint(min_len, max_len)
        start = 0 if r == 0 else max(0, n_pos - length) if r == n_reads - 1 else rng.randrange(max(1, n_pos - min_len + 1) if max_start is None else max_start + 1)
        idx = list(range(start, min(n_pos, start + length)))
        kept = [p for p in idx if p in (0, n_pos - 1) or rng.random() <= p_keep] or idx[:1]
        reads.append([(p, rng.choice(alleles_at[p]) if rng.random() < p_err else haps[h][p]) for p in kept])
    return reads


def n_genotypes(ploidy, n_alleles):
    n = 1
    for k in range(1, n_alleles):
        n = n * (ploidy + k) // k
    return n


def edge_cases(rng):
    cases = []
    # nan: candidates; main() keeps the ones for which the reference reports NaN scores.  The recipe "three alleles, ploidy 6, err = 0"
    # (the estimate becomes 0.0) never gives one: with err = 0.0 every position with two or more alleles has a genotype of likelihood
    # log(0), the exp overflows, the depths are halved down to one allele and every term is log(1) = 0 (several hundred variants of it
    # over ploidy 2 - 8, 3 - 5 alleles and err 0, 0.2 - 1.0 were run: no NaN, a third of the err = 0 ones with estimate 0.0).  What does
    # give NaN scores is an err whose square overflows: (1 - err) * err and err * err are then -inf and +inf, their sums NaN for the
    # allele pairs that meet both and +inf for the others.  Near 3e153 ... 1e154 only the longer sums overflow: NaN and stored pairs.
    for ploidy, n_alleles, err in ((3, 3, float("inf")), (4, 2, 1e154), (6, 3, 3e153), (6, 3, 4e153), (4, 3, 5e153), (6, 2, 6e153),
                                   (3, 3, 8e153), (2, 2, 1e160), (6, 3, 2.5e153), (4, 3, 3e153), (6, 3, 0.0), (6, 3, 0.0), (4, 3, 0.0)):
        reads = haplotype_reads(rng, 25, 12, ploidy, n_alleles, 2, 8, p_err=0.1)
        cases.append(dict(kind="nan", ploidy=ploidy, min_overlap=rng.choice((1, 2)), err=err, reads=reads))
    # high_ploidy: with two alleles fracAlt = index / ploidy runs over every multiple of 1 / ploidy
    for ploidy, n_alleles in ((7, 2), (8, 2), (10, 2), (12, 2), (15, 2), (8, 3), (10, 3)):
        reads = haplotype_reads(rng, 30, 25, ploidy, n_alleles, 2, 12)
        for err in (0.0, 0.07):
            cases.append(dict(kind="high_ploidy", ploidy=ploidy, min_overlap=rng.choice((1, 2, 3)), err=err, reads=reads))
    # many_alleles: max_allele 5 - 16 (the stride of the term table); two to five alleles at a position, five to eight where err = 0.2
    # (1 - err * (n_ex - 1) is then 0.2, 0, negative)
    for max_allele, ploidy in [(a, p) for a in (5, 8, 9, 15, 16) for p in (2, 3)] + [(5, 4), (8, 4), (9, 4)]:
        assert n_genotypes(ploidy, max_allele) <= 1000
        for err in (0.0, 0.07, 0.2):
            n_pos = 16
            sizes = (5, min(8, max_allele)) if err == 0.2 else (2, 5)
            alleles_at = [rng.sample(range(max_allele), rng.randint(*sizes)) for _ in range(n_pos)]
            alleles_at[rng.randrange(n_pos)][0] = max_allele - 1
            alleles_at = [sorted(set(a)) for a in alleles_at]
            reads = indexed_reads(rng, 40, n_pos, ploidy, alleles_at, 3, 10, p_err=0.3)
            assert max(a for r in reads for _, a in r) == max_allele - 1
            reads = [[(100 + 7 * p, a) for p, a in r] for r in reads]
            cases.append(dict(kind="many_alleles", ploidy=ploidy, min_overlap=rng.choice((1, 2)), err=err, reads=reads))
    # sparse_positions: few entries over many megabases (the sort-and-search branch), one case ending just below 2^31, and the two
    # sides of the threshold itself
    for n_reads, span, top, ploidy, n_alleles, err in ((30, 5_000_000, None, 2, 2, 0.07), (80, 50_000_000, None, 4, 2, 0.0),
                                                       (150, 200_000_000, None, 3, 3, 0.07), (60, 120_000_000, 2**31 - 1, 4, 3, 0.07),
                                                       (50, "at", None, 4, 2, 0.07), (50, "above", None, 4, 2, 0.07)):
        n_pos = n_reads // 2 + 10
        reads = indexed_reads(rng, n_reads, n_pos, ploidy, [list(range(n_alleles))] * n_pos, 2, 10)
        n_entries = sum(len(r) for r in reads)
        if span == "at":
            span = 64 * n_entries + BITMAP_SLACK       # the largest span that still takes the bitmap
        elif span == "above":
            span = 64 * n_entries + BITMAP_SLACK + 1   # the smallest one that is sorted
        lo = top - span + 1 if top else rng.randrange(1, 1_000_000)
        where = [lo] + sorted(rng.sample(range(lo + 1, lo + span - 1), n_pos - 2)) + [lo + span - 1]
        reads = [[(where[p], a) for p, a in r] for r in reads]
        cases.append(dict(kind="sparse_positions", ploidy=ploidy, min_overlap=rng.choice((1, 2)), err=err, reads=reads))
    # long_overlap: stored scores that are sums of hundreds to thousands of terms
    for ploidy, n_alleles, mo, err in ((4, 2, 1, 0.07), (6, 3, 300, 0.07), (4, 3, 300, 0.0), (6, 2, 1, 0.0)):
        n_pos = 3200
        reads = indexed_reads(rng, 24, n_pos, ploidy, [list(range(n_alleles))] * n_pos, 500, 1200, p_keep=0.98, p_err=0.02, max_start=600, n_long=3, long_len=3000)
        reads = [[(1000 + 3 * p, a) for p, a in r] for r in reads]
        cases.append(dict(kind="long_overlap", ploidy=ploidy, min_overlap=mo, err=err, reads=reads))
    return cases


def write_edge(exe, tmp):
    cases = edge_cases(random.Random(20261021))
    run(exe, cases, tmp)
    cases = [c for c in cases if c["kind"] != "nan" or c["nans"] > 0]
    nan = [c for c in cases if c["kind"] == "nan"]
    assert len(nan) >= 3 and any(c["expected"]["i"] for c in nan), "the reference gave too few NaN cases"
    with open(OUT_EDGE, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0) as f:   # (no time stamp: the same bytes on every run)
        f.write(json.dumps({"cases": cases}, separators=(",", ":")).encode())
    for kind in sorted({c["kind"] for c in cases}):
        of = [c for c in cases if c["kind"] == kind]
        print(f"{kind}: {len(of)} cases, {sum(1 for c in of if c['nans'] > 0)} with NaN scores, {sum(len(c['expected']['i']) for c in of)} entries")
    print(f"{len(cases)} cases -> {OUT_EDGE} ({os.path.getsize(OUT_EDGE)} bytes)")


def records_getters(c):
    return len(c["reads"]) <= 200 and c["kind"] != "long_overlap"   # (a long_overlap case's rows would double its size)


def run(exe, cases, tmp):
    lines = [str(len(cases))]
    for c in cases:
        getters = 1 if records_getters(c) else 0
        lines.append(f"{c['ploidy']} {c['min_overlap']} {float(c['err']).hex()} {len(c['reads'])} {getters}")
        for r in c["reads"]:
            lines.append(" ".join([str(len(r))] + [f"{p} {a}" for p, a in r]))
    out = os.path.join(tmp, "out.txt")
    subprocess.run([exe, out], input="\n".join(lines) + "\n", text=True, check=True, stdout=subprocess.DEVNULL)
    text = open(out).read().split("\n")
    k = 0
    for c in cases:
        m = re.match(r"case (\S+) (\d+) (\d+)", text[k])
        k += 1
        c["err_used"] = float.fromhex(m.group(1))
        c["nans"] = int(m.group(2))
        n = int(m.group(3))
        ent = [tuple(int(x) for x in text[k + t].split()) for t in range(n)]
        k += n
        c["expected"] = {"i": [e[0] for e in ent], "j": [e[1] for e in ent], "bits": [e[2] for e in ent]}
        if records_getters(c):
            g = {}
            for _ in range(6):
                head, *vals = text[k].split()
                k += 1
                g[head] = [int(v) for v in vals]
            rows, vals, x = [], g.pop("rows"), 0
            while x < len(vals):
                cnt = vals[x]
                rows.append([[vals[x + 1 + 2 * t], vals[x + 2 + 2 * t]] for t in range(cnt)])
                x += 1 + 2 * cnt
            g["rows"] = rows
            g["maxallele"] = g["maxallele"][0]
            c["getters"] = g
        c["reads"] = [[list(e) for e in r] for r in c["reads"]]


def main():
    args = [a for a in sys.argv[1:] if a != "--edge"]
    edge = len(args) != len(sys.argv) - 1   # --edge: write polyphase_edge_cases.json.gz, leave polyphase_cases.json.gz as it is
    ref_root = args[0] if args else os.environ.get("WHATSHAP_REFERENCE", "")
    if not ref_root or not os.path.isdir(os.path.join(ref_root, "src", "polyphase")):
        sys.exit("usage: make_polyphase_golden.py [--edge] /path/to/reference (a WhatsHap source tree)")
    if edge:
        with tempfile.TemporaryDirectory() as tmp:
            write_edge(build_driver(ref_root, tmp), tmp)
        return
    rng = random.Random(20261016)
    cases = small_cases(rng) + special_cases(rng) + medium_cases(rng)
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(ref_root, tmp)
        run(exe, cases, tmp)
    with gzip.open(OUT, "wt") as f:
        json.dump({"cases": cases}, f, separators=(",", ":"))
    print(f"{len(cases)} cases, {sum(len(c['expected']['i']) for c in cases)} entries, "
          f"{sum(c['nans'] for c in cases)} NaN scores -> {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
