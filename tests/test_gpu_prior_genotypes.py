"""GPU: the prior genotype likelihoods (whatshap_amd.genotype, csrc/priorgt_device.hip) against every value recorded from the reference
and, on problems the reference was not run on, against the one-thread host twin of the debug library: identical bytes.  The runs at
every class boundary and the 1 300-entry column with its subnormal are among the recorded cases; the launch constant; two calls on one
input byte for byte; the shim's round trip."""
import os
import re
import types

import numpy as np
import pytest

import prior_genotype_cases as pc
from whatshap_amd import _native, core, shim
from whatshap_amd import genotype as gt

pytestmark = pytest.mark.gpu

GOLDEN = pc.load_golden()
BY_NAME = {c["name"]: c for c in GOLDEN}
FIELDS = ("gl", "genotype", "reg", "reg_genotype")
COUNTS = ("n_reads", "n_positions", "n_entries", "n_counted", "n_covered", "n_genotyped", "columns_class_a", "columns_class_b", "columns_class_c", "longest_run")
_HEADER = open(os.path.join(os.path.dirname(os.path.abspath(gt.__file__)), "..", "include", "whatshap_amd.h")).read()
LAUNCHES = int(re.search(r"#define WHAMD_PRIOR_GENOTYPES_LAUNCHES (\d+)u", _HEADER).group(1))


def hexes(array):
    return [pc.hex3(row) for row in array.tolist()]


def same(got, want):
    for field in FIELDS:
        assert getattr(got, field).tobytes() == getattr(want, field).tobytes(), field
    assert {k: got.stats[k] for k in COUNTS} == {k: want.stats[k] for k in COUNTS}


def test_device_equals_every_recorded_value():
    """All recorded cases as one call, then the deep ones alone (a batch of one)."""
    results = gt.prior_genotypes_batch([pc.problem_of(c) for c in GOLDEN])
    for case, res in zip(GOLDEN, results):
        name = case["name"]
        assert hexes(res.gl) == case["gl"], name
        assert res.genotype.tolist() == case["gt"], name
        if case["constant"] is not None:
            assert hexes(res.reg) == case["reg"], name
            assert res.reg_genotype.tolist() == case["reg_gt"], name
        assert res.stats["launches"] == LAUNCHES
    stats = {c["name"]: r.stats for c, r in zip(GOLDEN, results)}
    assert stats["run_64"]["columns_class_a"] == 1 and stats["run_65"]["columns_class_b"] == 1
    assert stats["run_1024"]["columns_class_b"] == 1 and stats["run_1025"]["columns_class_c"] == 1
    assert stats["run_4097"]["columns_class_c"] == 1 and stats["run_4097"]["longest_run"] == 4097
    for name in ("run_1025", "run_4097", "deep_ref_q30"):
        alone = gt.prior_genotypes_batch([pc.problem_of(BY_NAME[name])])[0]
        assert hexes(alone.gl) == BY_NAME[name]["gl"], name


def test_the_subnormal_of_the_deep_column():
    """1 300 reads of allele 0, quality 30: the device's f64 division and subnormals give the reference's (1.0, 1e-323, 0.0)."""
    res = gt.prior_genotypes_batch([pc.problem_of(BY_NAME["deep_ref_q30"])])[0]
    print("device:", pc.hex3(res.gl[0]), "reference:", BY_NAME["deep_ref_q30"]["gl"][0])
    assert pc.hex3(res.gl[0]) == BY_NAME["deep_ref_q30"]["gl"][0] == pc.hex3((1.0, 1e-323, 0.0))


def test_device_equals_the_host_twin_on_a_fresh_batch():
    problems = [pc.problem_of(c) for c in pc.fresh_batch(7, 64)]
    dev, host = gt.prior_genotypes_batch(problems), gt.prior_genotypes_batch(problems, host=True)
    for d, h in zip(dev, host):
        same(d, h)
    assert sum(d.stats["n_counted"] for d in dev) > 2_000


def test_the_number_of_launches_is_the_headers_constant():
    assert LAUNCHES == _native.PRIOR_GENOTYPES_LAUNCHES
    cases = pc.fresh_batch(9, 64)
    one = gt.prior_genotypes_batch([pc.problem_of(cases[0])])[0]
    assert one.stats["n_counted"] > 0 and one.stats["launches"] == LAUNCHES
    assert all(r.stats["launches"] == LAUNCHES for r in gt.prior_genotypes_batch([pc.problem_of(c) for c in cases]))
    hollow = [pc.problem_of(BY_NAME[name]) for name in ("none_counted", "no_reads", "no_positions")]
    for problems in ([], hollow[:1], hollow):
        for res in gt.prior_genotypes_batch(problems):
            assert res.stats["launches"] == 0 and res.stats["n_counted"] == 0
    # ... and such a problem inside a call with others is answered like alone
    mixed = gt.prior_genotypes_batch([pc.problem_of(cases[1]), hollow[0], pc.problem_of(cases[2]), hollow[1]])
    assert hexes(mixed[1].gl) == BY_NAME["none_counted"]["gl"] and hexes(mixed[3].gl) == BY_NAME["no_reads"]["gl"]
    assert hexes(mixed[3].reg) == BY_NAME["no_reads"]["reg"] and mixed[3].reg_genotype.tolist() == BY_NAME["no_reads"]["reg_gt"]
    assert mixed[0].stats["launches"] == LAUNCHES


def test_two_calls_on_one_input_give_identical_bytes():
    """The order inside a placed run is whatever the atomics gave; after the ordering it must not show.  Reads of several entries over
    few positions: every column's run is filled by many workgroups at once."""
    cases = [pc.run_case(50_021, position=50)]   # (amplicon depth: the last class at tens of thousands of entries)
    reads = [[(p, (r + p) % 3 % 2, pc.QUALITIES[(r * 7 + p) % 9]) for p in range(r % 5, r % 5 + 12)] for r in range(3_000)]
    reads.sort(key=lambda read: read[0][0])
    cases.append(pc.from_reads("wide", reads, list(range(0, 16)), constant=1e-3, gt_qual_threshold=10))
    problems = [pc.problem_of(c) for c in cases]
    first, second = (gt.prior_genotypes_batch(problems) for _ in range(2))
    host = gt.prior_genotypes_batch(problems, host=True)
    for a, b, h in zip(first, second, host):
        for field in FIELDS:
            assert getattr(a, field).tobytes() == getattr(b, field).tobytes(), field
        same(a, h)
    assert (first[1].stats["columns_class_b"], first[1].stats["columns_class_c"]) == (2, 14)


def test_more_scan_tiles_than_one_pass_of_the_second_scan_launch():
    """2048 * 512 + 1 positions are 513 scan tiles: the one workgroup that scans the tile totals takes 256 per pass, so it carries over
    twice and its last pass holds a single tile with a single column.  Almost every column is empty.  Counted entries lie on both sides
    of the first tile's end (2047 | 2048), of the first pass's end (524 287 | 524 288) and of the last full tile's end (1 048 575 |
    1 048 576); a class b run (65) and a class c run (1 025) lie inside the last full tile, so their list entries, and the run begins
    behind them, come from the second pass.  300 entries of allele 2, which are not counted, fall anywhere."""
    n_col, last_full = 2048 * 512 + 1, 2048 * 511
    keys = np.array([0, 2047, 2048, 2049, 524_287, 524_288, last_full + 100, last_full + 1000, 1_048_575, 1_048_576])
    runs = np.array([3, 1, 2, 5, 7, 1, 65, 1025, 4, 6])
    rng = np.random.default_rng(5)
    n_counted, n_other = int(runs.sum()), 300
    pos = np.concatenate([np.repeat(keys, runs), rng.integers(0, n_col, size=n_other)])
    allele = np.concatenate([rng.integers(0, 2, size=n_counted), np.full(n_other, 2)])
    order = np.argsort(pos, kind="stable")   # reads of one entry each, in the order of their positions
    problem = gt.PriorProblem(np.arange(pos.size + 1), pos[order], allele[order], rng.integers(0, 40, size=pos.size), np.arange(n_col), constant=1e-3,
                              gt_prob=0.9, want_regularized=True)
    dev, host = gt.prior_genotypes_batch([problem])[0], gt.prior_genotypes_batch([problem], host=True)[0]
    same(dev, host)
    s = dev.stats
    assert s["n_positions"] == n_col and s["n_counted"] == n_counted and s["n_covered"] == keys.size and s["launches"] == LAUNCHES
    assert (s["columns_class_b"], s["columns_class_c"], s["longest_run"]) == (1, 1, 1025)


def test_shim_round_trip():
    case = BY_NAME["random_1002"]

    def original(readset, positions=None):
        raise AssertionError("the stand-in's own compute_genotypes was called")

    module = types.SimpleNamespace(compute_genotypes=original)
    previous = shim.install_genotype_priors(module)
    assert module.compute_genotypes is not original and previous.bindings == {"compute_genotypes": original}
    genotypes, gls = module.compute_genotypes(pc.readset_of(case, core), case["positions"])
    assert [pc.hex3(g) for g in gls] == case["gl"]
    assert genotypes == [gt.int_to_diploid_biallelic_gt(g) for g in case["gt"]]
    previous.restore()
    assert module.compute_genotypes is original
