"""CPU: the planner's head hook (csrc/slots.h SlotPlanHead, DESIGN.md 6.1 "The preview").  A lone table's create asks plan_forward_slots to finish the steps
of the table's preview FIRST and to call back, launches those runs from the callback, and lets the planner finish the rest under them.  Two things must hold,
and both are held here without a device, through whamd_debug_head_first_plan of the debug library:

* the plan does not depend on the hook: a digest over steps, runs (all 192 bytes of each: in_pos / out_pos, flags, bases), the rows and backtrace columns of
  every run, control words, ending and starting slots, exit slots and the component list is the same at every head size 1 .. pieces - 1 and without the hook;
* inside the callback the head is finished: the digest of runs [0, S), their rows, control words, ending slots and backtrace columns, taken inside the callback,
  equals the digest of the same part of the finished plan -- the planner's second half writes nothing a launched run was given --, and the callback is made once.

Tables: 2 and 4 plan pieces of 8 192 columns at coverage 6 - 9: regular, tie-heavy, homozygous columns (their runs leave Y form, so the `in` / `out` flags of
the neighbours differ) inside the head, in the last run of the head and in the first run behind it, two connected components cut inside the head, irregular."""
import numpy as np
import pytest

from whatshap_amd import _native
from whatshap_amd._native import ProblemArrays
from whatshap_amd.synthetic import irregular_block, synthetic_block

PIECE = 8192
Y, Y_IN, Y_OUT = 1, 2, 4   # SlotRun::yflags: the run computes in Y form, its entering column is in Y form, its exit column stays in Y form


def tie_heavy(p):
    p.var_quality[:] = 1
    return p


def with_homozygous_columns(p, columns):
    for c in columns:
        p.genotype.reshape(-1)[c] = 0 if c % 2 else 2   # a run that holds such a column leaves Y form
    return p


def cut_before(p, column):
    """The same table without the reads that span the boundary in front of `column`: a second connected component begins there."""
    first = p.positions[column]
    lengths = np.diff(p.read_ptr).astype(np.int64)
    begin, end = p.read_ptr[:-1].astype(np.int64), p.read_ptr[1:].astype(np.int64)
    ok = ~((p.var_position[begin] < first) & (p.var_position[end - 1] >= first))
    keep = np.repeat(ok, lengths)
    read_ptr = np.zeros(int(ok.sum()) + 1, dtype=np.uint64)
    read_ptr[1:] = np.cumsum(lengths[ok])
    return ProblemArrays(read_ptr, p.var_position[keep], p.var_allele[keep], p.var_quality[keep], p.read_sample_id[ok], p.individual_id, p.triple_ids,
                         p.genotype, None, p.recombcost, p.positions, False, n_variants=p.n_variants)


# name -> (pieces, maker); the homozygous tables name the head size whose edge their columns sit at
TABLES = {
    "regular_2_cov6": (2, lambda: synthetic_block(n_variants=2 * PIECE, coverage=6, seed=81)),
    "regular_4_cov9": (4, lambda: synthetic_block(n_variants=4 * PIECE, coverage=9, seed=82)),
    "tie_heavy_2_cov8": (2, lambda: tie_heavy(synthetic_block(n_variants=2 * PIECE, coverage=8, seed=83))),
    "tie_heavy_4_cov7": (4, lambda: tie_heavy(synthetic_block(n_variants=4 * PIECE, coverage=7, seed=84))),
    "homozygous_inside_head_2_cov8": (2, lambda: with_homozygous_columns(synthetic_block(n_variants=2 * PIECE, coverage=8, seed=85), (700, 701, 3000))),
    "homozygous_last_head_run_2_cov7": (2, lambda: with_homozygous_columns(synthetic_block(n_variants=2 * PIECE, coverage=7, seed=86), (PIECE - 3,))),
    "homozygous_first_run_behind_2_cov9": (2, lambda: with_homozygous_columns(synthetic_block(n_variants=2 * PIECE, coverage=9, seed=87), (PIECE + 2,))),
    "homozygous_last_head_run_4_cov8": (4, lambda: with_homozygous_columns(synthetic_block(n_variants=4 * PIECE, coverage=8, seed=88), (2 * PIECE - 3,))),
    "homozygous_first_run_behind_4_cov6": (4, lambda: with_homozygous_columns(synthetic_block(n_variants=4 * PIECE, coverage=6, seed=89), (2 * PIECE + 2,))),
    "two_components_2_cov8": (2, lambda: cut_before(synthetic_block(n_variants=2 * PIECE, coverage=8, seed=90), 3000)),
    "two_components_4_cov9": (4, lambda: cut_before(synthetic_block(n_variants=4 * PIECE, coverage=9, seed=91), 5000)),
    "irregular_2_cov9": (2, lambda: irregular_block(n_variants=2 * PIECE, coverage=9, seed=92)),
    "irregular_4_cov8": (4, lambda: irregular_block(n_variants=4 * PIECE, coverage=8, seed=93)),
}
_plans = {}


def plans(name):
    """The plan of the table without the hook and at every head size: made once, shared."""
    if name not in _plans:
        pieces, make = TABLES[name]
        p = make()
        _plans[name] = [_native.debug_head_first_plan(p, h) for h in range(pieces)]
    return _plans[name]


@pytest.mark.parametrize("name", list(TABLES))
def test_the_plan_does_not_depend_on_the_head(name):
    pieces = TABLES[name][0]
    plain, *hooked = plans(name)
    assert plain["n_pieces"] == pieces and plain["hook_calls"] == 0 and plain["head_steps"] == 0 and plain["n_runs"] > 100, plain
    for h, r in enumerate(hooked, start=1):
        assert r["digest"] == plain["digest"], (h, r, plain)
        assert (r["n_steps"], r["n_runs"], r["n_components"]) == (plain["n_steps"], plain["n_runs"], plain["n_components"]), (h, r, plain)


@pytest.mark.parametrize("name", list(TABLES))
def test_the_head_is_finished_inside_the_callback(name):
    plain, *hooked = plans(name)
    before = 0
    for h, r in enumerate(hooked, start=1):
        assert r["hook_calls"] == 1, (h, r)
        assert r["head_digest_in_hook"] == r["head_digest"], (h, r)
        assert 0 < r["head_steps"] < r["n_steps"] and r["head_steps"] >= before, (h, r, before)   # (every table here begins with slot runs)
        if not name.startswith("irregular"):   # (an irregular layout has per-column steps between its runs: the head ends at the first of them)
            assert r["head_steps"] > before, (h, r, before)
        before = r["head_steps"]


def test_the_component_cut_lies_inside_the_head():
    for name in ("two_components_2_cov8", "two_components_4_cov9"):
        assert all(r["n_components"] == 2 for r in plans(name)), plans(name)
    assert all(r["n_components"] == 1 for r in plans("regular_4_cov9"))


@pytest.mark.parametrize("name,h", [("homozygous_last_head_run_2_cov7", 1), ("homozygous_last_head_run_4_cov8", 2)])
def test_the_last_run_of_the_head_is_not_in_y_form(name, h):
    last, behind = plans(name)[h]["edge_yflags"]
    assert last is not None and behind is not None and not last & Y, (last, behind)
    assert behind & Y and not behind & Y_IN, (last, behind)   # (its entering column is converted: the neighbour's flag was read across the edge)


@pytest.mark.parametrize("name,h", [("homozygous_first_run_behind_2_cov9", 1), ("homozygous_first_run_behind_4_cov6", 2)])
def test_the_first_run_behind_the_head_is_not_in_y_form(name, h):
    last, behind = plans(name)[h]["edge_yflags"]
    assert last is not None and behind is not None and not behind & Y, (last, behind)
    assert last & Y and not last & Y_OUT, (last, behind)   # (the head's last run converts its exit column: it read the flag of a run finished later)


def test_a_regular_edge_stays_in_y_form():
    last, behind = plans("regular_4_cov9")[2]["edge_yflags"]
    assert last & Y and last & Y_OUT and behind & Y and behind & Y_IN, (last, behind)
