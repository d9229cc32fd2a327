"""GPU (-m gpu): WHICH kernel instantiation every launch of a solve takes (the launch ledger of the debug library, include/whatshap_amd_debug.h,
DESIGN.md 6.2), next to WHAT it computes.  Every problem of this file is solved through libwhatshap_amd_debug.so with no debug switch set -- the
choices are the product's -- and

(a) its result equals the oracle's, in full;
(b) its launches are consistent: the forward records add up to stats()["forward_launches"], no launch asks for more than 160 KiB of LDS, a launch
    above 64 KiB names a kernel of the large-LDS opt-in, no block has more than 1 024 threads, a run launched on its own has run.threads threads;
(c) every record's kernel is the one expected_kernels() below gives for the record's facts -- literal tables written from DESIGN.md 4 - 6.2, slots.h and the
    comments of launch_slot_run; it does not call the library and does not mirror its index arithmetic;
(d) the closing test: the kernels launched by this file are exactly the registry's entries that are not debug-only (less EXCLUDED, with reasons).

A swap inside a selection table that is still exact (packed <-> staged, Y form where the plain form is right too, tight <-> loose, XC = 32 where 8
was meant) changes no result; it fails (c).  An instantiation nothing reaches fails (d).  A new instantiation goes into the registry
(dp_device.hip solve_kernels), into the rule's tables, and into a problem of this file."""

import numpy as np
import pytest

import oracle
from helpers import first_difference, table_solution
from whatshap_amd import _native
from whatshap_amd.synthetic import irregular_block, random_small_instance, synthetic_block

pytestmark = pytest.mark.gpu

KIB = 1024

# ---------------------------------------------------------------------------------------------------------------- (c) the rule
# per-column kernels: one instantiation per (transmission values T, individuals NIND)
COLUMN_PAIRS = [(1, 1), (1, 2), (1, 3), (1, 4), (1, 5), (1, 6), (4, 3), (4, 4), (4, 5), (4, 6), (16, 4), (16, 5), (16, 6)]
# pedigree slot runs (slots.h): TB = log2 T; NF = cost forms per transmission value -- 2, 4 or 16, or a factorised line (untrusted genotypes)
PSLOT_FACT, PSLOT_FACT4 = 1, 3
PEDSLOT_ROWS = {(2, 2): "2, 2", (2, 4): "2, 4", (4, 2): "4, 2", (4, 4): "4, 4", (2, 16): "2, 16", (2, PSLOT_FACT): "2, PSLOT_FACT", (4, PSLOT_FACT4): "4, PSLOT_FACT4"}
# X runs of four cells per thread: the prologue forms the operands of XC columns -- the run's length rounded up to 8; 0: streamed operands
XC_OF_COLUMNS = [(range(1, 9), 8), (range(9, 17), 16), (range(17, 25), 24), (range(25, 33), 32)]
# group launches (enum GroupVariant): value -> kernel; the single-individual variants have a form held to four workgroups per CU
GROUP_KERNELS = {
    0: {False: "slot_group<2, false, false>", True: "slot_group<2, false, true>"},
    1: "pedslot_group<2, 2>", 2: "pedslot_group<2, 4>", 3: "pedslot_group<4, 2>", 4: "pedslot_group<4, 4>", 5: "pedslot_group<2, 16>",
    6: {False: "slot_group<3, false, false>", True: "slot_group<3, false, true>"},
    7: "pedslot_group<2, PSLOT_FACT>", 8: "slot_groupx<2, false>", 9: "slot_groupx<3, false>", 10: "pedslot_group<4, PSLOT_FACT4>",
}
TAIL_KERNELS = {"tail": {"backtrace_kernel", "backtrace_chunks", "backtrace_gather", "superreads_single"}, "window_walk": {"backtrace_kernel"},
                "group_walk": {"backtrace_chunks_group", "backtrace_gather_group", "superreads_group"}, "tables": {"ped_tables", "resident_tables"}}


def _b(v):
    return "true" if v else "false"


def expected_kernels(r):
    """The kernel names the rule allows for a ledger record (one name, except for the two launches of a keys column and the tails)."""
    site = r["site"]
    if site == "column":
        assert (r["T"], max(r["n_ind"], 1)) in COLUMN_PAIRS or r["wide"]
        if r["mode"] == 0:
            assert not r["wide"]
            return {f"column_step_fused<{r['T']}, {max(r['n_ind'], 1)}>"}
        return {"column_step_wide" if r["wide"] else f"column_step_keys<{r['T']}, {max(r['n_ind'], 1)}>", "column_finalize"}
    if site == "run":   # LDS-resident runs (path "resident"): the complement symmetry / the chunked backtrace's speculation
        if r["ped"]:
            return {"resident_segment_ped<false, true>" if r["spec"] else "resident_segment_ped<false>"}
        return {f"resident_segment<false, {_b(r['sym'])}>"}
    if site == "slot_run":
        if r["ped"]:   # PACKED: SlotRun::yflags bit 4
            assert r["pack"] == (1 if r["yflags"] & 16 else 0)
            return {f"pedslot_run<{PEDSLOT_ROWS[(r['tb'], r['nf'])]}, {_b(r['spec'])}, {_b(r['yflags'] & 16)}>"}
        if (r["yflags"] & 8) and r["lr"] == 2:   # X run with four cells per thread
            xc = 0 if r["streamed"] else next(v for cols, v in XC_OF_COLUMNS if r["ncols"] in cols)
            return {f"slot_runx<2, {xc}, false, {_b(r['spec'])}>"}
        assert r["lr"] in (1, 2, 3) and not (r["lr"] == 1 and r["yflags"] & 1)
        return {f"slot_run<{r['lr']}, false, {_b(r['spec'])}, {_b(r['yflags'] & 1)}>"}
    if site == "batch":
        return {f"slot_batch<{r['lr']}>"} if r["lr"] is not None else {f"resident_batch<{_b(r['sym'])}>"}
    if site == "group":
        k = GROUP_KERNELS[r["variant"]]
        return {k[bool(r["tight"])] if isinstance(k, dict) else k}
    return TAIL_KERNELS[site]


def rule_range():
    """Every name the rule can give: what the registry's non-debug entries must equal (tests/test_abi.py checks it without a device)."""
    names = {"column_step_wide", "column_finalize"}
    for t, n in COLUMN_PAIRS:
        names |= {f"column_step_fused<{t}, {n}>", f"column_step_keys<{t}, {n}>"}
    names |= {"resident_segment_ped<false, true>", "resident_segment_ped<false>", "resident_segment<false, false>", "resident_segment<false, true>",
              "resident_batch<false>", "resident_batch<true>", "slot_batch<1>", "slot_batch<2>", "slot_batch<3>"}
    for row in PEDSLOT_ROWS.values():
        names |= {f"pedslot_run<{row}, {s}, {p}>" for s in ("true", "false") for p in ("true", "false")}
    for xc in (0, 8, 16, 24, 32):
        names |= {f"slot_runx<2, {xc}, false, {s}>" for s in ("true", "false")}
    for lr, y in ((1, "false"), (2, "false"), (2, "true"), (3, "false"), (3, "true")):
        names |= {f"slot_run<{lr}, false, {s}, {y}>" for s in ("true", "false")}
    for k in GROUP_KERNELS.values():
        names |= set(k.values()) if isinstance(k, dict) else {k}
    for s in TAIL_KERNELS.values():
        names |= s
    return names


# (d) instantiations no input reaches: name -> reason (DESIGN.md 6.2 lists them too).  A launch of one of them fails the closing test.
EXCLUDED = {}

LAUNCHED = set()      # kernel names over every problem of this file
TESTS_RUN = set()     # the tests of this file that ran to their end (the closing test needs all of them)
LAST_LEDGER = []      # the ledger check_ledger read last


# ---------------------------------------------------------------------------------------------------------------- solving with the ledger
class debug_library:
    """Every table made inside goes through libwhatshap_amd_debug.so (as test_superreads_made_on_the_device_equal_the_hosts_loop does it)."""

    def __enter__(self):
        self.saved = _native._lib
        _native.use_debug_library()

    def __exit__(self, *exc):
        _native._lib = self.saved


_registry = None


def registry():
    global _registry
    if _registry is None:
        _registry = {k["name"]: k for k in _native.debug_solve_kernels()}
    return _registry


def check_ledger(table, what, alone=True):
    """(b) and (c) for one solved table; returns the names it launched."""
    stats, ledger = table.stats(), _native.debug_launches(table)
    LAST_LEDGER[:] = ledger
    reg = registry()
    assert sum(r["count"] for r in ledger if r["forward"]) == stats["forward_launches"], (what, stats["forward_launches"], ledger)
    names = set()
    for r in ledger:
        assert not r["stamps"], (what, r)   # (None or 0: no debug switch is set)
        assert r["lds"] <= 160 * KIB and r["block"] <= 1024, (what, r)
        assert r["lds"] <= 64 * KIB or reg[r["name"]]["large_lds_opted_in"], (what, "more than 64 KiB of LDS through a kernel outside the opt-in", r)
        assert not reg[r["name"]]["debug_only"], (what, r)
        if r["site"] in ("run", "slot_run"):
            assert r["block"] == r["threads"], (what, r)
        if r["site"] == "slot_run" and not r["ped"] and (r["yflags"] & 8) and r["lr"] == 2:
            # narrow X runs are packed onto one XCD (eight times the grid); a table running beside others, or 1 024 workgroups wide, streams its operands
            grid = r["grid_x"] // 8 if r["pack"] else r["grid_x"]
            assert bool(r["pack"]) == (grid <= 32 and not r["streamed"]), (what, r)
        if alone:
            assert r["own_stream"], (what, r)
        allowed = expected_kernels(r)
        assert r["name"] in allowed, (what, "the rule gives", sorted(allowed), "the launch took", r)
        names.add(r["name"])
    keys = sum(r["count"] for r in ledger if r["site"] == "column" and r["mode"] != 0 and r["name"] != "column_finalize")
    assert keys == sum(r["count"] for r in ledger if r["name"] == "column_finalize"), (what, "every keys column is finalized once")
    LAUNCHED.update(names)
    print("LEDGER", what, sorted(names))   # (pytest -s: the kernels of every table, for profiles/kernel_ledger/README.md)
    return names


_oracle_cache = {}


def oracle_solution(problem, key):
    if key not in _oracle_cache:
        _oracle_cache[key] = table_solution(oracle.OracleTable(problem))
    return _oracle_cache[key]


def solve_and_check(problem, key, path=None, **options):
    """One table alone through the debug library: (a), (b), (c).  Returns (names launched, stats)."""
    want = oracle_solution(problem, key)
    with debug_library():
        t = _native.NativeTable(problem, solve=False, path=path, options={k: str(v) for k, v in options.items()})
        t.solve()
        got = table_solution(t)
        what = (key, path, options)
        assert got == want, (what, first_difference(want, got))
        names = check_ledger(t, what)
        stats = t.stats()
        t.close()
    return names, stats


def solve_many_and_check(members, against_oracle=None, grouped=None):
    """One enqueue_many of (key, problem, options) through the debug library.  The members whose position is in `against_oracle` (default: all) are
    held to the oracle, the rest to their solve alone.  grouped: whether every member must (True) or must not (False) have shared its launches.
    Returns (names launched per member, stats per member)."""
    with debug_library():
        tables = [_native.NativeTable(p, solve=False, options={k: str(v) for k, v in opts.items()}) for _, p, opts in members]
        _native.enqueue_many(tables)
        _native.wait_many(tables)
        names, stats = [], []
        for i, ((key, p, opts), t) in enumerate(zip(members, tables)):
            got = table_solution(t)
            if against_oracle is None or i in against_oracle:
                want = oracle_solution(p, key)
            else:
                alone = _native.NativeTable(p, options={k: str(v) for k, v in opts.items()})
                want = table_solution(alone)
                alone.close()
            assert got == want, (key, first_difference(want, got))
            stats.append(t.stats())
            if grouped is not None:
                assert (stats[-1]["group_tables"] == len(tables)) == grouped and (grouped or stats[-1]["group_tables"] == 1), (key, stats[-1])
            names.append(check_ledger(t, key, alone=False))
        for t in tables:
            t.close()
    return names, stats


def _variant_of(p, quality=None, genotype=None, recomb=None):
    return _native.ProblemArrays(p.read_ptr, p.var_position, p.var_allele, p.var_quality if quality is None else quality, p.read_sample_id, p.individual_id,
                                 p.triple_ids, p.genotype.reshape(p.n_individuals, p.n_variants) if genotype is None else genotype,
                                 None if p.genotype_likelihoods is None else p.genotype_likelihoods.reshape(p.n_individuals, p.n_variants, 3),
                                 p.recombcost if recomb is None else recomb, p.positions, p.distrust_genotypes, n_variants=p.n_variants)


FAMILY_READS = [(0, 6), (0, 7), (1, 7), (1, 8), (2, 8), (2, 9), (7, 9), (8, 9)]   # (first, last variant): coverage 6 over variants 2 .. 6


def family(n_unrelated, triples, seed):
    """A small table of trusted all-heterozygous genotypes: the individuals of `triples` (father, mother, child, ...) and n_unrelated more.  Ten variants,
    eight reads dealt round robin to the individuals, coverage 6 at the most -- and six reads that all go on to the next column in columns 2 .. 5: the
    smallest column the fused kernel takes (64 projection entries); the other columns take the keys kernel on either path."""
    rng = np.random.default_rng(seed)
    n_ind = (max(triples) + 1 if triples else 0) + n_unrelated
    n_variants = 10
    read_ptr, pos, allele, quality = [0], [], [], []
    for first, last in FAMILY_READS:
        for v in range(first, last + 1):
            pos.append(10 * (v + 1)); allele.append(int(rng.integers(0, 2))); quality.append(int(rng.choice([1, 2, 7, 30])))
        read_ptr.append(len(pos))
    sample = [i % n_ind for i in range(len(FAMILY_READS))]
    recomb = rng.choice(np.array([1, 2, 5, 12], dtype=np.uint32), size=n_variants)
    return _native.ProblemArrays(read_ptr, pos, allele, quality, sample, np.arange(n_ind, dtype=np.uint32), np.asarray(triples, dtype=np.uint32),
                                 np.ones((n_ind, n_variants), dtype=np.uint8), None, recomb, 10 * (np.arange(n_variants, dtype=np.uint32) + 1), False, n_variants=n_variants)


TRIO, QUARTET, TWO_TRIOS = [0, 1, 2], [0, 1, 2, 0, 1, 3], [0, 1, 2, 3, 4, 5]
FAMILIES = {(1, n): (n, []) for n in range(1, 7)}
FAMILIES.update({(4, 3 + n): (n, TRIO) for n in range(4)})
FAMILIES.update({(16, 4): (0, QUARTET), (16, 5): (1, QUARTET), (16, 6): (0, TWO_TRIOS)})


# ---------------------------------------------------------------------------------------------------------------- the problems
@pytest.mark.parametrize("pair", COLUMN_PAIRS, ids=lambda p: f"T{p[0]}_NIND{p[1]}")
def test_per_column_kernels(pair):
    """column_step_fused<T, NIND> (path "column") and column_step_keys<T, NIND> + column_finalize (path "column_keys") for each of the thirteen pairs."""
    unrelated, triples = FAMILIES[pair]
    p = family(unrelated, triples, seed=100 * pair[0] + pair[1])
    t, n = pair
    fused, _ = solve_and_check(p, ("family", pair), path="column")
    assert f"column_step_fused<{t}, {n}>" in fused, fused
    keys, _ = solve_and_check(p, ("family", pair), path="column_keys")
    assert {f"column_step_keys<{t}, {n}>", "column_finalize"} <= keys and not any(k.startswith("column_step_fused") for k in keys), keys
    TESTS_RUN.add(f"test_per_column_kernels[{pair}]")


def test_column_step_wide():
    """Two parents and three children (T = 64): no templated kernel, the generic one."""
    import random

    rng = random.Random(191)
    solved = 0
    while solved < 3:
        p = random_small_instance(rng, mode="three_children", max_variants=8, max_reads=7, allow_conflict=False)
        try:
            oracle_solution(p, ("three_children", solved))
        except oracle.OracleError:
            _oracle_cache.pop(("three_children", solved), None)
            continue
        names, _ = solve_and_check(p, ("three_children", solved))
        assert "column_step_wide" in names, names
        solved += 1
    TESTS_RUN.add("test_column_step_wide")


def single(n_variants, coverage, seed, kind="plain", **kw):
    """A single-individual block; kind "heavy": weights beyond the packed evaluation and some homozygous columns (no Y form)."""
    p = synthetic_block(n_variants=n_variants, coverage=coverage, seed=seed, **kw)
    if kind == "heavy":
        rng = np.random.default_rng(seed)
        p = _variant_of(p, quality=p.var_quality * np.uint32(450), genotype=rng.choice([0, 1, 1, 2], size=(1, p.n_variants)).astype(np.uint8))
    return p


@pytest.mark.parametrize("slot_r", [1, 2, 3])
def test_slot_runs_of_a_single_individual(slot_r):
    """slot_run<LR, false, SPEC, YFORM>: two, four and eight cells per thread; Y form (weights as generated) and not (heavy weights, homozygous columns);
    SPEC where the table is long enough for the chunked backtrace (more than 2 x BT_CHUNK_RUNS units: 900 columns in runs of 11) and not (120)."""
    seen = set()
    for kind in ("plain", "heavy"):
        for n in (120, 900):
            p = single(n, 12, 40, kind, step=1)
            names, stats = solve_and_check(p, ("single", n, kind), slot_r=slot_r)
            assert (stats["bt_chunks"] > 0) == (n == 900), (n, stats)
            seen |= names
    want = {f"slot_run<{slot_r}, false, {s}, false>" for s in ("true", "false")}
    if slot_r == 3:   # (four cells in Y form: X runs, or runs too long for them -- test_x_runs; two cells have no Y form)
        want |= {"slot_run<3, false, true, true>", "slot_run<3, false, false, true>"}
    assert want <= seen, sorted(want - seen)
    TESTS_RUN.add(f"test_slot_runs_of_a_single_individual[{slot_r}]")


def test_x_runs():
    """slot_runx<2, XC, false, SPEC>: runs of up to 8, 16, 24 and 32 columns (reads one, two variants apart: runs of 11 and 22 columns; irregular layouts:
    every length), SPEC and not, packed onto one XCD (grid <= 32) and not (coverage 18 without the symmetry: 128 workgroups); and slot_run<2, ..., true>,
    the Y form of four cells per thread, where a run (33 columns: reads three variants apart) is too long for the X kernel's registers."""
    seen = set()
    for step, n in ((1, 120), (1, 900), (2, 120), (2, 900), (3, 200), (3, 1300)):
        names, _ = solve_and_check(single(n, 12, 60 + step, step=step), ("x", step, n))
        seen |= names
    for seed, n, cov in X_IRREGULAR:
        names, _ = solve_and_check(irregular_block(n, cov, seed=seed), ("irregular", seed, n, cov))
        seen |= names
    with debug_library():
        t = _native.NativeTable(single(40, 18, 80, step=1), options={"symmetry": "0"})
        assert table_solution(t) == oracle_solution(single(40, 18, 80, step=1), ("wide", 40, 0))
        seen |= check_ledger(t, "wide alone")
        assert any(r["grid_x"] == 128 and r["pack"] == 0 and r["streamed"] == 0 for r in _native.debug_launches(t)), _native.debug_launches(t)
        t.close()
    want = {f"slot_runx<2, {xc}, false, {s}>" for xc in (8, 16, 24, 32) for s in ("true", "false")} | {"slot_run<2, false, true, true>", "slot_run<2, false, false, true>"}
    assert want <= seen, sorted(want - seen)
    TESTS_RUN.add("test_x_runs")


X_IRREGULAR = [(7, 1500, 13), (8, 1500, 12), (9, 150, 13)]


def test_streamed_x_runs_side_by_side():
    """Tables that keep their own streams in one enqueue_many take the streamed X kernel (XC = 0): two of coverage 18 (128 workgroups wide each, too few and
    too wide for a group), and -- for SPEC -- a long one beside a table that no group takes (two cells per thread)."""
    wide = [(("wide", 40, i), single(40, 18, 80 + i, step=1), {"symmetry": 0}) for i in range(2)]
    names, _ = solve_many_and_check(wide, grouped=False)
    assert all("slot_runx<2, 0, false, false>" in s for s in names), names
    pair = [(("x", 1, 900), single(900, 12, 61, step=1), {}), (("single", 120, "plain"), single(120, 12, 40, step=1), {"slot_r": 1})]
    names, stats = solve_many_and_check(pair, grouped=False)
    assert "slot_runx<2, 0, false, true>" in names[0] and stats[0]["bt_chunks"] > 0, (names, stats)
    TESTS_RUN.add("test_streamed_x_runs_side_by_side")


def components(n_blocks, n_variants, coverage, seed):
    """A single-individual ReadSet of n_blocks connected components with the SAME read layout (synthetic_block's layout does not depend on the seed; alleles
    and weights do): on as many lanes the components advance in lockstep, so every super-step batches runs of one shape -- the symmetric ones too."""
    parts = [synthetic_block(n_variants, coverage, seed=seed + b) for b in range(n_blocks)]
    ptr, pos, positions, offset, base = [np.zeros(1, np.uint64)], [], [], 0, 0
    for p in parts:
        pos.append(p.var_position + offset)
        positions.append(p.positions + offset)
        ptr.append(p.read_ptr[1:] + np.uint64(base))
        base += int(p.read_ptr[-1])
        offset = int(positions[-1][-1]) + 1000
    ptr = np.concatenate(ptr)
    return _native.ProblemArrays(ptr, np.concatenate(pos), np.concatenate([p.var_allele for p in parts]), np.concatenate([p.var_quality for p in parts]),
                                 np.zeros(ptr.size - 1, np.int32), [0], [], np.ones((1, n_blocks * n_variants), dtype=np.uint8), None,
                                 np.concatenate([p.recombcost for p in parts]), np.concatenate(positions), False)


@pytest.mark.parametrize("symmetry", [0, 2])
def test_batched_runs_of_many_components(symmetry):
    """A ReadSet of four components on several lanes: slot_batch<1 / 2 / 3> (path "auto") and resident_batch<false / true> (path "resident")."""
    p = components(4, 60, 13, seed=11)   # (coverage 13: runs of two and more workgroups, the least the complement symmetry halves)
    seen = set()
    for slot_r in (1, 2, 3):
        names, _ = solve_and_check(p, ("components", 13), lanes=4, slot_r=slot_r, symmetry=symmetry)
        assert f"slot_batch<{slot_r}>" in names, names
        seen |= names
    names, _ = solve_and_check(p, ("components", 13), path="resident", lanes=4, symmetry=symmetry)
    assert f"resident_batch<{_b(symmetry)}>" in names, names
    TESTS_RUN.add(f"test_batched_runs_of_many_components[{symmetry}]")


@pytest.mark.parametrize("symmetry", [0, 2])
def test_lds_resident_runs(symmetry):
    """Path "resident": resident_segment<false, SYM> of a single individual; resident_segment_ped<false> of a short trio and <false, true> of one long
    enough for the chunked backtrace."""
    def largest_run_lds():   # what the launches of the table solved last asked for, against what the plan check approved (res_segment_lds_bytes on both sides)
        return max(r["lds"] for r in LAST_LEDGER if r["site"] == "run")

    names, _ = solve_and_check(single(120, 13, 90), ("resident single", 120), path="resident", symmetry=symmetry)   # (two workgroups per run)
    assert f"resident_segment<false, {_b(symmetry)}>" in names, names
    assert largest_run_lds() == _native.plan_summary(single(120, 13, 90), "resident")["max_lds_bytes"]
    trio = synthetic_block(n_variants=120, coverage=8, seed=91, trio=True)
    short, _ = solve_and_check(trio, ("resident trio", 120), path="resident", symmetry=symmetry)
    assert "resident_segment_ped<false>" in short, short
    assert largest_run_lds() == _native.plan_summary(trio, "resident")["max_lds_bytes"]
    long, stats = solve_and_check(synthetic_block(n_variants=2000, coverage=8, seed=92, trio=True), ("resident trio", 2000), path="resident", symmetry=symmetry)
    assert "resident_segment_ped<false, true>" in long and stats["bt_chunks"] > 0, (long, stats)
    TESTS_RUN.add(f"test_lds_resident_runs[{symmetry}]")


def pedigree(row, n_variants, seed, staged=False):
    """A table whose pedigree slot runs take row (TB, NF) of PEDSLOT_ROWS; staged: recombination costs that leave no room for packed keys."""
    tb, nf = row
    kw = dict(n_variants=n_variants, coverage=8, seed=seed)
    if row == (2, PSLOT_FACT) or row == (2, 16):
        kw.update(trio=True, distrust_genotypes=True)
    elif row == (4, PSLOT_FACT4):
        kw.update(quartet=True, distrust_genotypes=True)
    elif tb == 2:
        kw.update(trio=True)
    elif nf == 2:
        kw.update(quartet=True)
    else:
        kw.update(two_trios=True)   # (four founders, all heterozygous: the children's constraints leave four of the sixteen allele assignments)
    p = synthetic_block(**kw)
    if row == (2, 4):   # a trio and one unrelated individual: three founders, the child's constraint leaves four of the eight assignments
        sample = (np.arange(p.n_reads) % 4).astype(np.int32)
        p = _native.ProblemArrays(p.read_ptr, p.var_position, p.var_allele, p.var_quality, sample, np.arange(4, dtype=np.uint32), p.triple_ids,
                                  np.ones((4, p.n_variants), dtype=np.uint8), None, p.recombcost, p.positions, False, n_variants=p.n_variants)
    if staged:
        # the table's upper bound (about 2 x trios x recombination cost per column) between 2^(31 - TB), where packed keys end, and the 2^30 slot runs need
        big = int(2 ** (29.5 if tb == 2 else 28.5) / (2 * (len(p.triple_ids) // 3) * n_variants))
        rng = np.random.default_rng(seed)
        p = _variant_of(p, recomb=rng.choice(np.array([big, big - 1, big // 2], dtype=np.uint32), size=p.recombcost.size))
    return p


@pytest.mark.parametrize("row", list(PEDSLOT_ROWS), ids=lambda r: PEDSLOT_ROWS[r].replace(", ", "_"))
def test_pedigree_slot_runs(row, monkeypatch):
    """pedslot_run<TB, NF, SPEC, PACKED>, all four of each row: a table short and one long enough for the chunked backtrace, with recombination costs
    as generated (packed keys) and so large that the staged step runs."""
    if row == (2, 16):
        monkeypatch.setenv("WHAMD_NO_PED_FACT", "1")   # (a switch of the product: sixteen forms instead of the factorised line)
    seen = set()
    for n, spec in ((100, False), (900, True)):
        for staged in (False, True):
            names, stats = solve_and_check(pedigree(row, n, 200 + 10 * row[0] + row[1], staged), ("pedigree", row, n, staged))
            assert stats["forward_launches"] <= n // 3, "the table did not run on pedigree slot runs"
            assert (stats["bt_chunks"] > 0) == spec, (n, stats)
            seen |= names
    want = {f"pedslot_run<{PEDSLOT_ROWS[row]}, {s}, {k}>" for s in ("true", "false") for k in ("true", "false")}
    assert want <= seen, sorted(want - seen)
    TESTS_RUN.add(f"test_pedigree_slot_runs[{row}]")


def group_members():
    """Small tables of every kind a group launch has a variant for: (key, problem, options)."""
    shared = {"shared_launches": 1}
    members = [(("g single", 0), single(120, 12, 300, step=1), shared), (("g single", 1), single(90, 8, 301), shared), (("g heavy", 0), single(100, 12, 302, "heavy", step=1), shared),
               (("g single8", 0), single(100, 12, 303, step=1), dict(shared, slot_r=3)), (("g heavy8", 0), single(100, 12, 304, "heavy", step=1), dict(shared, slot_r=3))]
    for i, row in enumerate(r for r in PEDSLOT_ROWS if r != (2, 16)):
        members.append((("g ped", row), pedigree(row, 90, 310 + i), shared))
    return members


def test_group_launches_loose(monkeypatch):
    """One enqueue_many of small tables of mixed kinds: every GroupVariant in its loose form; long members: the batched backtrace and superreads_group."""
    seen = set()
    names, _ = solve_many_and_check(group_members(), grouped=True)
    for s in names:
        seen |= s
    long = [(("x", 1, 900), single(900, 12, 61, step=1), {}), (("single", 900, "heavy"), single(900, 12, 40, "heavy", step=1), {}), (("pedigree", (2, 2), 900, False), pedigree((2, 2), 900, 222), {})]
    names, stats = solve_many_and_check(long, grouped=True)
    assert all(s["bt_chunks"] > 0 for s in stats), stats
    for s in names:
        seen |= s
    monkeypatch.setenv("WHAMD_NO_PED_FACT", "1")   # (a switch of the product: sixteen forms instead of the factorised line)
    names, _ = solve_many_and_check([(("g ped16", i), pedigree((2, 16), 90, 330 + i), {}) for i in range(2)], grouped=True)
    for s in names:
        seen |= s
    want = {k[False] if isinstance(k, dict) else k for k in GROUP_KERNELS.values()} | TAIL_KERNELS["group_walk"]
    assert want <= seen, sorted(want - seen)
    TESTS_RUN.add("test_group_launches_loose")


def test_group_launches_tight():
    """Eighteen members of coverage 18 with heavy weights (no X runs), 64 workgroups wide with four cells per thread and 32 with eight (the layout of a wide
    table that is told it shares its launches: every other member), pass 768 workgroups together: slot_group<2 / 3, false, true>.  Two against the oracle,
    the rest against their solve alone."""
    members = [(("g tight", i), single(30, 18, 400 + i, "heavy", step=1), {"shared_launches": i % 2}) for i in range(18)]
    names, _ = solve_many_and_check(members, against_oracle={0, 1}, grouped=True)
    seen = set().union(*names)
    want = {"slot_group<2, false, true>", "slot_group<3, false, true>"}
    assert want <= seen, sorted(want - seen)
    TESTS_RUN.add("test_group_launches_tight")


def test_windowed_walk():
    """An arena limit below the table's records: the solve runs in windows, each walked by backtrace_kernel right behind its steps."""
    names, _ = solve_and_check(single(1000, 12, 500, step=1), ("windowed", 1000), arena_limit_bytes=1 << 17)
    assert "backtrace_kernel" in names and any(r["site"] == "window_walk" for r in LAST_LEDGER), LAST_LEDGER
    TESTS_RUN.add("test_windowed_walk")


# ---------------------------------------------------------------------------------------------------------------- (d) coverage
def all_test_ids():
    ids = [f"test_per_column_kernels[{p}]" for p in COLUMN_PAIRS] + ["test_column_step_wide"] + [f"test_slot_runs_of_a_single_individual[{r}]" for r in (1, 2, 3)]
    ids += ["test_x_runs", "test_streamed_x_runs_side_by_side"] + [f"test_batched_runs_of_many_components[{s}]" for s in (0, 2)]
    ids += [f"test_lds_resident_runs[{s}]" for s in (0, 2)] + [f"test_pedigree_slot_runs[{r}]" for r in PEDSLOT_ROWS]
    return ids + ["test_group_launches_loose", "test_group_launches_tight", "test_windowed_walk"]


def test_every_shipping_kernel_of_the_solve_was_launched():
    """The union of the kernels launched above == the registry's entries that are not debug-only, less EXCLUDED; nothing excluded was launched."""
    missing_tests = [t for t in all_test_ids() if t not in TESTS_RUN]
    if missing_tests:
        pytest.skip(f"needs every test of this file to have run and passed in this process; not run: {missing_tests[:4]} ...")
    shipping = {name for name, k in registry().items() if not k["debug_only"]}
    assert not (LAUNCHED & set(EXCLUDED)), sorted(LAUNCHED & set(EXCLUDED))
    assert set(EXCLUDED) <= shipping, sorted(set(EXCLUDED) - shipping)
    assert LAUNCHED | set(EXCLUDED) == shipping, ("never launched", sorted(shipping - LAUNCHED - set(EXCLUDED)), "not in the registry", sorted(LAUNCHED - shipping))
