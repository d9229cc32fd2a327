"""GPU (-m gpu): the users of the X runs' prologue (kernels_slots.h slot_runx_lds_core, slot_runx_stream_core) against the oracle, through the product library
and through the debug library with no debug switch set.  The order of the prologue's memory requests must not change a result:

* coverage 20, 96 columns: the ramp and two full-width unpacked runs of 22 columns -- 256 workgroups of eight waves, `slot_runx<2, 24>` -- with
  two-valued qualities, so that nearly every minimum is a tie and a cell that arrived late or stale shows in the index path;
* coverage 12, 300 columns: narrow runs packed onto one XCD;
* an irregular layout at coverage 15: runs of 8, 16 and 32 prologue columns, columns in which two and three reads end;
* three coverage-15 tables as one sequence of launches: the streamed `slot_groupx`.

Compared in full (helpers.table_solution): cost, index path, partitioning, superreads."""

import numpy as np
import pytest

import oracle
from helpers import first_difference, table_solution
from whatshap_amd import _native
from whatshap_amd.synthetic import irregular_block, synthetic_block

pytestmark = pytest.mark.gpu


def _two_valued(p, seed):
    """The same reads with qualities drawn from {1, 2}."""
    q = np.random.default_rng(seed).integers(1, 3, size=p.var_quality.size).astype(p.var_quality.dtype)
    return _native.ProblemArrays(p.read_ptr, p.var_position, p.var_allele, q, p.read_sample_id, p.individual_id, p.triple_ids,
                                 p.genotype.reshape(p.n_individuals, p.n_variants), None, p.recombcost, p.positions, p.distrust_genotypes, n_variants=p.n_variants)


PROBLEMS = {
    "cov20_ties": lambda: _two_valued(synthetic_block(96, 20, seed=3), 11),
    "cov12_packed": lambda: synthetic_block(300, 12, seed=5),
    "irregular_cov15": lambda: irregular_block(400, 15, seed=9),   # (this seed has runs of every XC; 80 columns in which two reads end, 34 with three or more)
    "group_0": lambda: synthetic_block(300, 15, seed=21),
    "group_1": lambda: synthetic_block(300, 15, seed=22),
    "group_2": lambda: synthetic_block(300, 15, seed=23),
}
_cache = {}


def case(name):
    """(problem, the oracle's solution): made once, shared by the two libraries' tests, never changed."""
    if name not in _cache:
        p = PROBLEMS[name]()
        _cache[name] = (p, table_solution(oracle.OracleTable(p)))
    return _cache[name]


class library:
    def __init__(self, debug):
        self.debug = debug

    def __enter__(self):
        self.saved = _native._lib
        if self.debug:
            _native.use_debug_library()
        else:
            _native._lib = None
            _native.lib()

    def __exit__(self, *exc):
        _native._lib = self.saved


def _x_launches(table):
    """(kernel name, grid_x, pack) of the X-run launches in the debug library's ledger."""
    return {(r["name"], r["grid_x"], bool(r.get("pack"))) for r in _native.debug_launches(table) if r["name"].startswith(("slot_runx", "slot_groupx"))}


@pytest.mark.parametrize("debug", [False, True], ids=["product", "debug"])
@pytest.mark.parametrize("name", ["cov20_ties", "cov12_packed", "irregular_cov15"])
def test_a_table_alone_equals_the_oracle(name, debug):
    p, want = case(name)
    with library(debug):
        t = _native.NativeTable(p, solve=False)
        t.solve()
        got = table_solution(t)
        launches = _x_launches(t) if debug else None
        t.close()
    assert got == want, (name, first_difference(want, got))
    if not debug:
        return
    names = {n for n, _, _ in launches}
    print("X launches", name, sorted(launches))
    if name == "cov20_ties":   # the flagship's kernel at its full width, one workgroup per CU
        assert ("slot_runx<2, 24, false, false>", 256, False) in launches, launches
    if name == "cov12_packed":   # (eight times the run's workgroups, every eighth works)
        assert any(pack for _, _, pack in launches), launches
    if name == "irregular_cov15":
        assert {f"slot_runx<2, {xc}, false, false>" for xc in (8, 16, 32)} <= names, names


@pytest.mark.parametrize("debug", [False, True], ids=["product", "debug"])
def test_three_tables_sharing_their_launches_equal_the_oracle(debug):
    members = [case(f"group_{i}") for i in range(3)]
    with library(debug):
        tables = [_native.NativeTable(p, solve=False) for p, _ in members]
        _native.enqueue_many(tables)
        _native.wait_many(tables)
        got = [table_solution(t) for t in tables]
        launches = [_x_launches(t) for t in tables] if debug else None
        for t in tables:
            t.close()
    for i, ((_, want), g) in enumerate(zip(members, got)):
        assert g == want, (i, first_difference(want, g))
    if debug:
        print("X launches of the group", [sorted(l) for l in launches])
        assert all(any(n.startswith("slot_groupx<2") for n, _, _ in l) for l in launches), launches
